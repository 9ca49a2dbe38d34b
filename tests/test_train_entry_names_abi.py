"""CPU-side checks of the names the three training entry ladders report under (rtxn_train_step*, rtxn_train_gradients*,
rtxn_volrender_*_train): every rung is called with nothing, with each option struct it accepts malformed in turn, and
-- a step -- with inactive structs over a batch without a model.  A rung whose own structs are absent is the rung below it, and
says so; a rung that holds its struct reports under its own name.  No device is touched: every rule is checked before one is."""
import ctypes as C

import pytest

P = C.c_void_p(4096)           # a fake device pointer: never launched from here

# (suffix, the option structs the rung accepts beside the sampler's jitter, in argument order)
STEP = [("", ()), ("_ex", ("bg",)), ("_jitter", ("bg",)), ("_loss", ("bg", "loss")), ("_reg", ("bg", "loss", "reg")),
        ("_opt", ("bg", "loss", "reg", "opt")), ("_scaled", ("bg", "loss", "reg", "opt", "scaler")),
        ("_ema", ("bg", "loss", "reg", "opt", "scaler", "ema")), ("_rays", ("bg", "loss", "reg", "opt", "scaler", "ema", "rays", "pose"))]
GRADIENTS = [("", ()), ("_ex", ("bg",)), ("_jitter", ("bg",)), ("_loss", ("bg", "loss")), ("_reg", ("bg", "loss", "reg")),
             ("_scaled", ("bg", "loss", "reg", "scaler")), ("_rays", ("bg", "loss", "reg", "scaler", "rays"))]
COMPOSITOR = [("l2_train", ()), ("l2_train_ex", ("bg",)), ("loss_train", ("bg", "loss")), ("reg_train", ("bg", "loss", "reg")),
              ("scaled_train", ("bg", "loss", "reg", "scaler"))]
# the name rule: what each rung reports under when every struct it accepts is NULL
STEP_NULL = {"": "rtxn_train_step", "_ex": "rtxn_train_step_ex", "_jitter": "rtxn_train_step_jitter", "_loss": "rtxn_train_step_loss",
             "_reg": "rtxn_train_step_reg", "_opt": "rtxn_train_step_reg", "_scaled": "rtxn_train_step_reg", "_ema": "rtxn_train_step_reg",
             "_rays": "rtxn_train_step_reg"}
GRADIENTS_NULL = {"": "rtxn_train_gradients", "_ex": "rtxn_train_gradients_ex", "_jitter": "rtxn_train_gradients_jitter",
                  "_loss": "rtxn_train_gradients_loss", "_reg": "rtxn_train_gradients_reg", "_scaled": "rtxn_train_gradients_reg",
                  "_rays": "rtxn_train_gradients_reg"}


# ---- the structs: valid (and, but for what the rungs above _reg require of each other, inactive), or with one field broken ------
def _bg(_lib, bad=False):
    s = _lib.TrainBackground()
    s.mode, s.target_channels = (7 if bad else 0), 3
    return s, b"background mode"


def _loss(_lib, bad=False):
    s = _lib.TrainLoss()
    s.kind = 99 if bad else 0
    return s, b"loss->kind"


def _reg(_lib, bad=False):
    s = _lib.TrainRegularizer()
    s.distortion_weight = -1.0 if bad else 0.0
    return s, b"distortion_weight"


def _opt(_lib, bad=False, on=True):
    """on: with the guard, lr_factor and the guard word, as the scaler and the EMA need them; else nothing switched on"""
    s = _lib.OptimizerOptions()
    s.schedule.ratio = 0.0 if bad else 1.0
    if on:
        s.skip_nonfinite, s.lr_factor, s.guard = 1, P, P
    return s, b"schedule.ratio"


def _scaler(_lib, bad=False):
    s = _lib.LossScaler()
    s.init_scale, s.growth, s.backoff, s.growth_interval, s.min_scale, s.max_scale = (100.0 if bad else 128.0), 2.0, 0.5, 2000, 1.0, 65536.0
    s.state, s.partials = P, P
    return s, b"init_scale"


def _ema(_lib, bad=False):
    s = _lib.WeightEma()
    s.decay, s.state, s.mlp_ema, s.table_ema, s.table_stamps = 0.9, P, (None if bad else P), P, P
    return s, b"mlp_ema"


def _rays(_lib, bad=False):
    s = _lib.RayGradients()
    for f in ("t_start", "t_end", "dstart", "dend", "d_origin", "d_direction"):
        setattr(s, f, P)
    if bad:
        s.t_start = None
    return s, b"rays->t_start"


def _pose(_lib, bad=False):
    s = _lib.PoseRefinement()
    s.n_images, s.lr, s.beta1, s.beta2, s.eps = 3, (-1e-3 if bad else 1e-3), 0.9, 0.999, 1e-15
    for f in ("poses0", "poses", "delta", "m", "v", "steps", "grad", "drawn"):
        setattr(s, f, P)
    return s, b"pose->lr"


MAKE = dict(bg=_bg, loss=_loss, reg=_reg, opt=_opt, scaler=_scaler, ema=_ema, rays=_rays, pose=_pose)


def _step_args(_lib, mlp=True):
    a = _lib.TrainStepArgs()
    a.batch.vr_mode, a.batch.sample_type, a.batch.loss_scale = 1, 3, 1.0
    a.batch.mlp, a.batch.grid = (P if mlp else None), (P if mlp else None)
    a.trace.mode, a.trace.rays_d = 1, P
    return a


def _call(_lib, ladder, suffix, accepts, first, structs):
    """the rung with `first` (its arguments before the option structs) and structs {name: struct or None}"""
    lib = _lib.lib()
    args = list(first)
    if ladder != "compositor" and suffix != "" and suffix != "_ex":
        accepts = accepts[:1] + ("jitter",) + accepts[1:]        # bg, jitter, loss, ...
    for name in accepts:
        s = structs.get(name)
        args.append(C.byref(s) if s is not None else None)
    fn = getattr(lib, {"step": "rtxn_train_step", "gradients": "rtxn_train_gradients", "compositor": "rtxn_volrender_"}[ladder] + suffix)
    rc = fn(*args, None)
    return rc, lib.rtxn_last_error()


# ---- (a) nothing at all -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix,accepts", STEP, ids=[s or "plain" for s, _ in STEP])
def test_a_step_rung_called_with_nothing_reports_under_the_lowest_rung_it_amounts_to(suffix, accepts):
    from rtx_nerf_amd import _lib
    rc, msg = _call(_lib, "step", suffix, accepts, [None], {})
    assert rc == 1 and msg == f"{STEP_NULL[suffix]}: NULL arguments".encode(), msg


@pytest.mark.parametrize("suffix,accepts", GRADIENTS, ids=[s or "plain" for s, _ in GRADIENTS])
def test_a_gradients_rung_called_with_nothing_reports_under_the_lowest_rung_it_amounts_to(suffix, accepts):
    from rtx_nerf_amd import _lib
    rc, msg = _call(_lib, "gradients", suffix, accepts, [None], {})
    want = "rtxn_train_gradients: NULL batch or model" if suffix == "" else f"{GRADIENTS_NULL[suffix]}: NULL batch"
    assert rc == 1 and msg == want.encode(), msg


@pytest.mark.parametrize("suffix,accepts", COMPOSITOR, ids=[s for s, _ in COMPOSITOR])
def test_a_compositor_rung_called_with_nothing_is_the_plain_compositor(suffix, accepts):
    """no struct is active, so the shared checks are rtxn_volrender_l2_train's: here the batch size, the first of them"""
    from rtx_nerf_amd import _lib
    rc, msg = _call(_lib, "compositor", suffix, accepts, [None, None, None, None, -1, 32, None, 1.0, None, None, None, None], {})
    assert rc == 1 and msg == b"rtxn_volrender_l2_train: batch_size = -1 < 0", msg


# ---- (b) one struct malformed, every other one valid ----------------------------------------------------------------------------
def _malformed_cases(ladder, rungs):
    return [pytest.param(ladder, suffix, accepts, bad, id=f"{ladder}{suffix or '_plain'}-{bad}")
            for suffix, accepts in rungs for bad in accepts]


@pytest.mark.parametrize("ladder,suffix,accepts,bad", _malformed_cases("step", STEP) + _malformed_cases("gradients", GRADIENTS) +
                         _malformed_cases("compositor", COMPOSITOR))
def test_a_rung_refuses_one_malformed_struct_under_its_own_name_and_names_the_field(ladder, suffix, accepts, bad):
    from rtx_nerf_amd import _lib
    structs, word = {}, None
    for name in accepts:
        structs[name], w = MAKE[name](_lib, bad=(name == bad))
        if name == bad:
            word = w
    args = _step_args(_lib)
    first = {"step": [C.byref(args)], "gradients": [C.byref(args.batch)],
             "compositor": [P, P, P, P, -1, 32, P, 1.0, P, P, P, P]}[ladder]
    rc, msg = _call(_lib, ladder, suffix, accepts, first, structs)
    own = {"step": "rtxn_train_step", "gradients": "rtxn_train_gradients", "compositor": "rtxn_volrender_"}[ladder] + suffix
    assert rc == 1 and msg.startswith(own.encode() + b": ") and word in msg, msg


# ---- (c) a step over inactive structs is the plain step ------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix,accepts", STEP, ids=[s or "plain" for s, _ in STEP])
def test_a_step_rung_over_inactive_structs_reaches_the_plain_steps_own_checks(suffix, accepts):
    """background NONE with 3 channels, L2 without an alpha term, weight 0 without outputs, options with nothing switched on;
    scaler, EMA, rays and pose NULL"""
    from rtx_nerf_amd import _lib
    structs = {"bg": _bg(_lib)[0], "loss": _loss(_lib)[0], "reg": _reg(_lib)[0], "opt": _opt(_lib, on=False)[0]}
    args = _step_args(_lib, mlp=False)
    rc, msg = _call(_lib, "step", suffix, accepts, [C.byref(args)], structs)
    assert rc == 1 and msg == b"rtxn_train_step: batch.mlp is NULL", msg
