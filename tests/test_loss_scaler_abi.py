"""CPU-side checks of the dynamic loss scale at the C-ABI boundary (rtxn_loss_scaler and the entry points that take it; DESIGN
5.14): symbols and bindings, the structs' layout against the C compiler, the rules every surface checks before any device is
touched, the Trainer (which raises before allocating), and the host twin of the device's state machine against a numpy
restatement written here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_loss_scaler_check", "rtxn_loss_scaler_workspace_bytes", "rtxn_loss_scaler_init_state", "rtxn_loss_scaler_advance",
               "rtxn_gradient_statistics", "rtxn_loss_scaler_step", "rtxn_adam_step_scaled", "rtxn_adam_step_sparse_scaled",
               "rtxn_volrender_scaled_train", "rtxn_train_gradients_scaled", "rtxn_train_step_scaled")
P = C.c_void_p(4096)           # a fake device pointer: never launched from here
F = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_loss_scaler_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    for n in ("loss_scaler", "loss_scaler_advance", "loss_scaler_state_tensor", "loss_scaler_workspace", "gradient_statistics",
              "loss_scaler_step", "adam_step_scaled", "adam_step_sparse_scaled", "volrender_scaled_train"):
        assert callable(getattr(api, n))
    import inspect
    assert "scaler" in inspect.signature(api.train_step).parameters and "scaler" in inspect.signature(api.train_gradients).parameters
    from rtx_nerf_amd.train import Trainer
    assert "max_grad_norm" in inspect.signature(Trainer.__init__).parameters
    assert lib.rtxn_loss_scaler_workspace_bytes() == 8 * 4 * api.GRAD_STATS_MAX_BLOCKS
    assert re.search(r"RTXN_GRAD_STATS_MAX_BLOCKS\s*=\s*%d\b" % api.GRAD_STATS_MAX_BLOCKS, _header())
    assert lib.rtxn_version() == 100


@pytest.mark.parametrize("name,T,fields,want", [
    ("rtxn_loss_scaler", "LossScaler", ["init_scale", "growth", "backoff", "growth_interval", "min_scale", "max_scale", "max_grad_norm",
                                        "state", "partials"], [48, 0, 4, 8, 12, 16, 20, 24, 32, 40]),
    ("rtxn_loss_scaler_state", "LossScalerState", ["scale", "multiplier", "good", "backoffs", "growths", "clipped", "grad_norm", "reserved"],
     [32, 0, 4, 8, 12, 16, 20, 24, 28])])
def test_struct_layouts_match_the_header_and_the_c_compiler(tmp_path, name, T, fields, want):
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    declared = []
    for d in body.split(";"):                       # `unsigned backoffs, growths, clipped` declares three
        if d.strip():
            declared += [re.findall(r"([A-Za-z_]\w*)\s*$", part.strip())[0] for part in d.split(",")]
    T = getattr(_lib, T)
    assert declared == [f[0] for f in T._fields_] == fields
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("' + "%zu " * (len(fields) + 1) + '\\n", '
                 f"sizeof({name}), " + ", ".join(f"offsetof({name}, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(c), "-o", str(exe)])
    got = [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == got == want


# ---- the rules -------------------------------------------------------------------------------------------------------------
_DEFAULTS = dict(init_scale=128.0, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=65536.0, max_grad_norm=0.0)
# (fields, the field the message names): each broken rule of include/rtxn.h, a non-power-of-two scale or factor among them
_REJECTED = [(dict(init_scale=100.0), b"init_scale"), (dict(init_scale=0.0), b"init_scale"), (dict(init_scale=-128.0), b"init_scale"),
             (dict(init_scale=float("inf")), b"init_scale"), (dict(init_scale=float("nan")), b"init_scale"),
             (dict(growth=3.0), b"growth"), (dict(growth=0.5), b"growth"), (dict(growth=1.5), b"growth"),
             (dict(backoff=0.3), b"backoff"), (dict(backoff=1.0), b"backoff"), (dict(backoff=0.0), b"backoff"), (dict(backoff=2.0), b"backoff"),
             (dict(min_scale=3.0), b"min_scale"), (dict(min_scale=0.0), b"min_scale"),
             (dict(max_scale=65535.0), b"max_scale"), (dict(max_scale=float("inf")), b"max_scale"),
             (dict(min_scale=256.0), b"min_scale = 256 <= init_scale = 128"), (dict(max_scale=64.0), b"init_scale = 128 <= max_scale = 64"),
             (dict(growth_interval=0), b"growth_interval"), (dict(growth_interval=-5), b"growth_interval"),
             (dict(max_grad_norm=-1.0), b"max_grad_norm"), (dict(max_grad_norm=float("inf")), b"max_grad_norm"),
             (dict(max_grad_norm=float("nan")), b"max_grad_norm")]


def _scaler(_lib, state=P, partials=P, **kw):
    s = _lib.LossScaler()
    for k, v in {**_DEFAULTS, **kw}.items():
        setattr(s, k, v)
    s.state, s.partials = state, partials
    return s


def _options(_lib, skip_nonfinite=1, lr_factor=P, guard=P):
    o = _lib.OptimizerOptions()
    o.schedule.ratio = 1.0
    o.skip_nonfinite, o.lr_factor, o.guard = skip_nonfinite, lr_factor, guard
    return o


def _surfaces(_lib, sc, opt=None):
    """(name, return code, message) of every entry point that takes the struct, on otherwise empty arguments: an accepted struct
    fails later, on the arguments' own checks or for want of a device"""
    lib = _lib.lib()
    args = _lib.TrainStepArgs()
    args.batch.vr_mode, args.batch.sample_type = 1, 3
    batch = _lib.TrainBatch()
    batch.vr_mode, batch.sample_type = 1, 3
    st = _lib.LossScalerState()
    st.scale = 128.0
    out = _lib.LossScalerState()
    bufs = (_lib.GradBuffer * 1)()
    bufs[0].count = -1
    s, o = C.byref(sc), C.byref(opt if opt is not None else _options(_lib))
    return [("rtxn_loss_scaler_check", lib.rtxn_loss_scaler_check(s), lib.rtxn_last_error()),
            ("rtxn_loss_scaler_init_state", lib.rtxn_loss_scaler_init_state(s, None), lib.rtxn_last_error()),
            ("rtxn_loss_scaler_advance", lib.rtxn_loss_scaler_advance(s, C.byref(st), 0, -1.0, 1.0, C.byref(out)), lib.rtxn_last_error()),
            ("rtxn_gradient_statistics", lib.rtxn_gradient_statistics(bufs, 1, P, s, None), lib.rtxn_last_error()),
            ("rtxn_loss_scaler_step", lib.rtxn_loss_scaler_step(o, s, bufs, 1, None, 1, 1e-3, 1e-2, 0.9, 0.999, None, None, 1.0, None),
             lib.rtxn_last_error()),
            ("rtxn_adam_step_scaled", lib.rtxn_adam_step_scaled(-1, P, P, P, 0, P, P, P, 1e-3, 0.9, 0.999, 1e-8, o, s, None), lib.rtxn_last_error()),
            ("rtxn_adam_step_sparse_scaled", lib.rtxn_adam_step_sparse_scaled(-1, P, P, P, 0, P, P, P, 1e-3, 0.9, 0.999, 1e-15, o, s, None),
             lib.rtxn_last_error()),
            ("rtxn_volrender_scaled_train", lib.rtxn_volrender_scaled_train(P, P, P, P, -1, 32, P, 0.0, P, P, P, P, None, None, None, s, None),
             lib.rtxn_last_error()),
            ("rtxn_train_gradients_scaled", lib.rtxn_train_gradients_scaled(C.byref(batch), None, None, None, None, s, None), lib.rtxn_last_error()),
            ("rtxn_train_step_scaled", lib.rtxn_train_step_scaled(C.byref(args), None, None, None, None, o, s, None), lib.rtxn_last_error())]


@pytest.mark.parametrize("kw,word", _REJECTED)
def test_every_surface_rejects_a_broken_rule_before_touching_a_device(kw, word):
    """RTXN_ERR_INVALID (1) and a message naming the field and the entry point, with or without a GPU"""
    from rtx_nerf_amd import _lib, api
    for name, rc, msg in _surfaces(_lib, _scaler(_lib, **kw)):
        assert rc == 1 and word in msg and name.encode() in msg, (name, rc, msg)
    with pytest.raises(_lib.RtxnError, match=re.escape(word.decode().split(" = ")[0])):
        api.loss_scaler(**kw)


def test_a_valid_scaler_reaches_the_arguments_own_checks_and_null_the_calls_without_it():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    got = {name: (rc, msg) for name, rc, msg in _surfaces(_lib, _scaler(_lib, max_grad_norm=1.0))}
    assert got["rtxn_loss_scaler_check"][0] == 0
    assert got["rtxn_loss_scaler_init_state"][0] == 1 and b"NULL state_out" in got["rtxn_loss_scaler_init_state"][1]
    assert got["rtxn_loss_scaler_advance"][0] == 1 and b"sumsq = -1" in got["rtxn_loss_scaler_advance"][1]
    assert got["rtxn_gradient_statistics"][0] == 1 and b"buffers[0].count" in got["rtxn_gradient_statistics"][1]
    assert got["rtxn_loss_scaler_step"][0] == 1 and b"rtxn_loss_scaler_step: step" in got["rtxn_loss_scaler_step"][1]
    assert got["rtxn_adam_step_scaled"][0] == 1 and b"rtxn_adam_step_scaled: n = -1" in got["rtxn_adam_step_scaled"][1]
    assert got["rtxn_adam_step_sparse_scaled"][0] == 1 and b"rtxn_adam_step_sparse_scaled: n = -1" in got["rtxn_adam_step_sparse_scaled"][1]
    assert got["rtxn_volrender_scaled_train"][0] == 1 and b"rtxn_volrender_scaled_train: batch_size = -1" in got["rtxn_volrender_scaled_train"][1]
    assert got["rtxn_train_gradients_scaled"][0] == 1 and b"NULL batch or model" in got["rtxn_train_gradients_scaled"][1]
    assert got["rtxn_train_step_scaled"][0] == 1 and b"batch.mlp is NULL" in got["rtxn_train_step_scaled"][1]
    # the device words: needed by everything that launches, not by the rules alone
    for kw in (dict(state=None), dict(partials=None)):
        for name, rc, msg in _surfaces(_lib, _scaler(_lib, **kw))[3:]:
            assert rc == 1 and b"scaler->state" in msg and name.encode() in msg, (name, rc, msg)
        assert _surfaces(_lib, _scaler(_lib, **kw))[0][1] == 0
    # dynamic scaling implies the non-finite guard
    for opt in (_options(_lib, skip_nonfinite=0), _options(_lib, guard=None), _options(_lib, lr_factor=None)):
        for name, rc, msg in _surfaces(_lib, _scaler(_lib), opt):
            if name in ("rtxn_loss_scaler_step", "rtxn_adam_step_scaled", "rtxn_adam_step_sparse_scaled", "rtxn_train_step_scaled"):
                assert rc == 1 and name.encode() in msg and (b"skip_nonfinite" in msg or b"opt->guard" in msg or b"opt->lr_factor" in msg), (name, msg)
    args = _lib.TrainStepArgs()
    args.batch.vr_mode, args.batch.sample_type = 1, 3
    assert lib.rtxn_train_step_scaled(C.byref(args), None, None, None, None, None, C.byref(_scaler(_lib)), None) == 1
    assert b"rtxn_train_step_scaled" in lib.rtxn_last_error() and b"skip_nonfinite" in lib.rtxn_last_error()
    # NULL scaler: the calls that existed before the struct, under their own names
    assert lib.rtxn_train_step_scaled(None, None, None, None, None, None, None, None) == 1 and b"rtxn_train_step_reg: NULL arguments" in lib.rtxn_last_error()
    assert lib.rtxn_train_gradients_scaled(None, None, None, None, None, None, None) == 1 and b"rtxn_train_gradients_reg: NULL batch" in lib.rtxn_last_error()
    # compat mode is refused with a message, as the regulariser refuses it
    args.batch.vr_mode = 0
    batch = _lib.TrainBatch()
    batch.vr_mode = 0
    assert lib.rtxn_train_step_scaled(C.byref(args), None, None, None, None, C.byref(_options(_lib)), C.byref(_scaler(_lib)), None) == 1
    assert b"RTXN_VR_NERF" in lib.rtxn_last_error() and b"rtxn_train_step_scaled" in lib.rtxn_last_error()
    assert lib.rtxn_train_gradients_scaled(C.byref(batch), None, None, None, None, C.byref(_scaler(_lib)), None) == 1
    assert b"RTXN_VR_NERF" in lib.rtxn_last_error() and b"rtxn_train_gradients_scaled" in lib.rtxn_last_error()


@pytest.mark.parametrize("kw,word", [(dict(loss_scale="auto"), "'dynamic'"), (dict(loss_scale=dict(init_scale=100.0)), "init_scale"),
                                     (dict(loss_scale=dict(growth=3.0)), "growth"), (dict(loss_scale=dict(backoff=0.3)), "backoff"),
                                     (dict(loss_scale=dict(growth_interval=0)), "growth_interval"),
                                     (dict(loss_scale=dict(init_scale=2.0, min_scale=4.0)), "min_scale"),
                                     (dict(loss_scale="dynamic", max_grad_norm=-1.0), "max_grad_norm"),
                                     (dict(max_grad_norm=float("inf")), "max_grad_norm"), (dict(max_grad_norm=float("nan")), "max_grad_norm"),
                                     (dict(loss_scale=100.0, max_grad_norm=1.0), "init_scale"),
                                     (dict(loss_scale="dynamic", mode="compat"), "mode='nerf'"),
                                     (dict(loss_scale=128.0, max_grad_norm=1.0, mode="compat"), "mode='nerf'")])
def test_trainer_refuses_bad_scaler_arguments_before_allocating(kw, word):
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match=re.escape(word)):
        Trainer(16, None, encoding="freq", device="cpu", **kw)


def test_trainer_refuses_the_three_launch_compositor(monkeypatch):
    from rtx_nerf_amd.train import Trainer
    monkeypatch.setenv("RTXN_TRAIN_FUSE_COMPOSITOR", "0")
    with pytest.raises(ValueError, match="RTXN_TRAIN_FUSE_COMPOSITOR=0"):
        Trainer(16, None, encoding="freq", device="cpu", loss_scale="dynamic")


# ---- the state machine, restated (include/rtxn.h, "dynamic loss scale") ---------------------------------------------------
def advance_np(cfg, st, flag, sumsq, D):
    """st: dict of the seven words; every float step in float32, the norm in float64 rounded once"""
    st = dict(st)
    s = F(st["scale"])
    if flag:
        st["scale"] = max(F(cfg["min_scale"]), F(s * F(cfg["backoff"])))
        st["good"] = 0
        st["backoffs"] += 1
        return st
    norm = F(np.sqrt(np.float64(sumsq)) / (np.float64(s) * np.float64(F(D))))
    mgn = F(cfg["max_grad_norm"])
    coef = min(F(1), F(mgn / F(norm + F(1e-6)))) if mgn > 0 else F(1)
    st["multiplier"] = F(coef * F(F(1) / F(s * F(D))))
    st["grad_norm"] = norm
    st["clipped"] += int(coef < 1)
    st["good"] += 1
    if st["good"] >= cfg["growth_interval"]:
        grown = min(F(cfg["max_scale"]), F(s * F(cfg["growth"])))
        st["good"] = 0
        st["growths"] += int(grown != s)
        st["scale"] = grown
    return st


_WORDS = ("scale", "multiplier", "good", "backoffs", "growths", "clipped", "grad_norm")


def _run(cfg, script, D):
    """the host twin and the restatement side by side over (flag, sumsq) steps; returns the states"""
    from rtx_nerf_amd import _lib, api
    sc = api.loss_scaler(**cfg)
    st = _lib.LossScalerState()
    assert _lib.lib().rtxn_loss_scaler_init_state(C.byref(sc), C.byref(st)) == 0
    want = dict(scale=F(cfg["init_scale"]), multiplier=F(1) / F(cfg["init_scale"]), good=0, backoffs=0, growths=0, clipped=0, grad_norm=F(0))
    seen = []
    for flag, sumsq in script:
        st = api.loss_scaler_advance(sc, st, flag, sumsq, D)
        want = advance_np(cfg, want, flag, sumsq, D)
        got = {w: getattr(st, w) for w in _WORDS}
        for w in _WORDS:
            assert F(got[w]).tobytes() == F(want[w]).tobytes() if w in ("scale", "multiplier", "grad_norm") else got[w] == want[w], (w, got, want)
        seen.append(got)
    return seen


@pytest.mark.parametrize("D", [1.0, 4.0])
def test_host_advance_matches_the_numpy_restatement(D):
    cfg = dict(_DEFAULTS, init_scale=64.0, growth=4.0, backoff=0.25, growth_interval=2, min_scale=2.0, max_scale=1024.0, max_grad_norm=0.5)
    s = lambda norm, scale: (norm * scale * D) ** 2              # the sum of squares of a gradient of that unscaled norm
    script = [(1, 0.0)] * 4                                      # 64 -> 16 -> 4 -> 2 (clamped from 1) -> 2
    script += [(0, s(0.1, 2.0)), (0, s(0.25, 2.0))]              # below the clip on the first, a growth after the second: 2 -> 8
    script += [(0, s(3.0, 8.0)), (1, 12.0), (0, s(0.7, 2.0))]    # a clip; a backoff that resets `good` (8 -> 2); a clip again
    script += [(0, s(0.4, 2.0))]                                 # good reaches 2: 2 -> 8
    script += [(0, 0.0)] * 12                                    # a zero gradient; growth to the max_scale clamp: 8 -> 32 -> 128 -> 512 -> 1024 -> 1024 -> 1024
    seen = _run(cfg, script, D)
    scales = [g["scale"] for g in seen]
    assert scales[:4] == [16.0, 4.0, 2.0, 2.0]                   # the min_scale clamp; the step at min_scale still counts as a backoff
    assert [g["backoffs"] for g in seen[:4]] == [1, 2, 3, 4]
    assert scales[4:6] == [2.0, 8.0] and [g["good"] for g in seen[4:6]] == [1, 0] and seen[5]["growths"] == 1
    assert [g["clipped"] for g in seen[4:10]] == [0, 0, 1, 1, 2, 2]           # the clip branch on both sides of 1
    assert seen[7]["scale"] == 2.0 and seen[7]["good"] == 0 and seen[7]["backoffs"] == 5 and seen[7]["multiplier"] == seen[6]["multiplier"]
    assert seen[8]["good"] == 1 and seen[9]["good"] == 0 and seen[9]["scale"] == 8.0
    assert scales[-1] == 1024.0 and scales[-3] == 1024.0
    assert seen[-1]["growths"] == seen[-3]["growths"] == 2 + 4   # at the clamp nothing changes: growths counts real changes only
    # a clipped step: the multiplier is coef / (s D) with coef = max_grad_norm / (norm + 1e-6)
    g = seen[6]
    assert abs(g["grad_norm"] - 3.0) < 1e-6 and abs(g["multiplier"] * 8.0 * D - 0.5 / 3.000001) < 1e-7


@pytest.mark.parametrize("D", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("scale", [1.0, 16.0, 128.0, 4096.0, 2.0 ** 40])
@pytest.mark.parametrize("max_grad_norm", [0.0, 1e3])
def test_without_a_clip_the_multiplier_is_exactly_one_over_scale_times_divisor(scale, D, max_grad_norm):
    cfg = dict(_DEFAULTS, init_scale=scale, min_scale=1.0, max_scale=2.0 ** 40, growth_interval=10 ** 6, max_grad_norm=max_grad_norm)
    seen = _run(cfg, [(0, (0.37 * scale * D) ** 2)], D)
    assert F(seen[0]["multiplier"]).tobytes() == (F(1) / F(F(scale) * F(D))).tobytes()
    assert seen[0]["clipped"] == 0 and seen[0]["scale"] == scale
