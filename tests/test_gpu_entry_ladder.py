"""Every rung of the three training entry ladders (rtxn_train_step*, rtxn_train_gradients*, rtxn_volrender_*_train)
called with nothing switched on -- its option structs NULL, or present and inactive -- is the plain entry point, bit for bit.
Deterministic mode keeps every sum order-independent, so the comparisons are torch.equal -- all but one scalar, whose sum is
not (_same)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_training_loop import _small_trainer

B = 900
MODELS = [("hash", "nerf", 64, 4),        # the recompute path
          ("freq", "compat", 128, 2)]     # saved activations, three compositor launches


def _inactive(api):
    """background NONE with 3 channels, L2 without an alpha term or opacity buffer, weight 0 without outputs, options with nothing
    switched on; the scaler, the EMA, the rays and the pose have no inactive form: NULL"""
    return dict(bg=api.train_background(None, target_channels=3), loss=api.train_loss("l2"), reg=api.train_regularizer(0.0),
                opt=api.optimizer_options())


def _rungs(prefix, ladder):
    """(symbol, the option arguments in order) per rung; jitter, scaler, ema, rays and pose are always NULL"""
    tail = {"": (), "_ex": ("bg",), "_jitter": ("bg", None), "_loss": ("bg", None, "loss"), "_reg": ("bg", None, "loss", "reg"),
            "_opt": ("bg", None, "loss", "reg", "opt"), "_scaled": ("bg", None, "loss", "reg", "opt", None),
            "_ema": ("bg", None, "loss", "reg", "opt", None, None), "_rays": ("bg", None, "loss", "reg", "opt", None, None, None, None)}
    if ladder == "gradients":
        tail = {k: tuple(x for x in v if x != "opt") for k, v in tail.items() if k not in ("_opt", "_ema")}
        tail["_rays"] = ("bg", None, "loss", "reg", None, None)
    return [(prefix + k, v) for k, v in tail.items()]


def _variants(api, ladder, prefix):
    """(label, symbol, arguments behind the first) for every rung: once with NULLs, once with inactive structs"""
    structs = _inactive(api)
    for sym, names in _rungs(prefix, ladder):
        yield f"{sym}(NULL)", sym, [None] * len(names)
        if any(names):
            yield f"{sym}(inactive)", sym, [C.byref(structs[n]) if n else None for n in names]


def _batch(torch):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
    t = torch.from_numpy(np.random.default_rng(7).uniform(0, 1, (B, 3)).astype(np.float32)).cuda()
    return o, d, t


def _same(torch, name, got, want, mode):
    """bit for bit -- but the loss scalar of the RTXN_VR_COMPAT route.  rtxn_l2_loss, its second launch, adds one partial sum per
    block (here 11: 2700 components, 256 per block) into the scalar with float atomics in whatever order the blocks retire, in
    deterministic mode too: two runs of rtxn_train_step ITSELF differ in its last bit.  Eleven non-negative partials summed in
    another order differ by at most 10 roundings of at most 2^-24 of the sum each."""
    if name == "loss" and mode == "compat":
        return abs(float(got) - float(want)) <= 10 * 2.0 ** -24 * float(want)
    return torch.equal(got, want)


def _state(tr):
    names = ["master", "params", "adam_m", "adam_v"] + (["table_master", "table", "table_m", "table_v", "table_steps"] if tr.encoding == "hash" else [])
    return {n: getattr(tr, n) for n in names}


@pytest.mark.gpu
@pytest.mark.parametrize("encoding,mode,neurons,layers", MODELS)
def test_every_step_rung_with_nothing_switched_on_is_the_plain_step(gpu, encoding, mode, neurons, layers):
    torch = gpu
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    tr = _small_trainer(torch, encoding, mode, neurons, layers, deterministic=True)
    assert tr._jitter(None) is None
    args = tr.entry_args(B, launch_segments=B * 30)
    o, d, t = _batch(torch)
    tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
    initial = {n: v.clone() for n, v in _state(tr).items()}
    want = None
    for label, sym, rest in _variants(api, "step", "rtxn_train_step"):
        for n, v in _state(tr).items():
            v.copy_(initial[n])
        tr.net.set_params_training(tr.params)
        tr.entry_step.zero_()
        tr._clear_grads()
        tr._det_select()
        for _ in range(2):
            _lib.check(getattr(lib, sym)(C.byref(args), *rest, api._stream()), sym)
        torch.cuda.synchronize()
        got = {n: v.clone() for n, v in _state(tr).items()}
        got["loss"] = tr.loss.clone()
        assert int(tr.entry_step.item()) == 2 and 0 < int(tr.total.item()) < B * 30
        if want is None:
            assert sym == "rtxn_train_step" and not torch.equal(got["master"], initial["master"]) and float(got["loss"]) > 0
            want = got
            continue
        for n in want:
            assert _same(torch, n, got[n], want[n], mode), f"{label}: {n} differs in {int((got[n] != want[n]).sum())} of {want[n].numel()} elements"


@pytest.mark.gpu
@pytest.mark.parametrize("encoding,mode,neurons,layers", MODELS)
def test_every_gradients_rung_with_nothing_switched_on_is_the_plain_call(gpu, encoding, mode, neurons, layers):
    torch = gpu
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    tr = _small_trainer(torch, encoding, mode, neurons, layers, deterministic=True)
    assert tr._jitter(None) is None
    o, d, t = _batch(torch)
    tr._det_select()
    P = tr._segments(o, d, B)
    assert 0 < P < B * 30
    hash_ = encoding == "hash"
    batch = api.train_batch(tr.net, grid=tr.hg if hash_ else None, n_dir_freqs=tr.hg.n_dir_freqs if hash_ else 0,
                            table=tr.table if hash_ else None, start_points=tr.start, end_points=tr.end, seg_view=tr.seg_view,
                            num_stored=tr.num_stored, indices=tr.indices, total_segments=tr.total, segment_capacity=B * 30, n_rays=B,
                            sample_type=tr._stype(None), t_scale=tr.density_scale if mode == "nerf" else 1.0,
                            vr_mode=api.VR_NERF if mode == "nerf" else api.VR_COMPAT, targets=t, loss_scale=tr.loss_scale, encT=tr.encT,
                            dencT=tr.dencT, workspace=tr.ws, output_half=tr.out, radiance=tr.radiance, t_vals=tr.t_vals,
                            radiance_gradients=tr.dout, pixels=tr.pixels, loss_gradients=tr.loss_grads, loss_sum=tr.loss,
                            dparams=tr.dparams, dtable=tr.dtable if hash_ else None,
                            dtable_hashed_half=tr.dtable_h if (hash_ and tr.hash_fp16) else None,
                            live_ws=tr.live_ws if tr.live_segments else None, workspace_lean=tr.lean)
    want = None
    for label, sym, rest in _variants(api, "gradients", "rtxn_train_gradients"):
        tr._clear_grads()
        tr.pixels.zero_()
        tr.loss.fill_(-1.0)
        _lib.check(getattr(lib, sym)(C.byref(batch), *rest, api._stream()), sym)
        torch.cuda.synchronize()
        got = dict(dparams=tr.dparams.clone(), pixels=tr.pixels.clone(), loss=tr.loss.clone())
        if hash_:
            got["table gradient"] = tr.table_grad()
        if want is None:
            assert sym == "rtxn_train_gradients" and float(got["dparams"].abs().max()) > 0 and float(got["loss"]) > 0
            assert not hash_ or float(got["table gradient"].abs().max()) > 0
            want = got
            continue
        for n in want:
            assert _same(torch, n, got[n], want[n], mode), f"{label}: {n} differs in {int((got[n] != want[n]).sum())} of {want[n].numel()} elements"


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 3], ids=["two-samples-per-lane", "one-sample-per-lane"])
def test_every_compositor_rung_with_nothing_switched_on_is_the_plain_compositor(gpu, K):
    """5 rays (a partial block of 4) with 0, 1, 3, 2 and 1 segments; K = 32 takes the pair kernels, the odd K = 3 the one-sample ones"""
    torch = gpu
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    shadow = api.deterministic_shadow(16)     # deterministic mode: the one-sample kernels add to the loss once per ray, in any order
    api.set_deterministic(shadow, None)
    try:
        _compositor_rungs(torch, _lib, api, lib, K)
    finally:
        api.release_deterministic(shadow, None)


def _compositor_rungs(torch, _lib, api, lib, K):
    hits = [0, 1, 3, 2, 1]
    n, S = len(hits), sum(hits) * K
    rng = np.random.default_rng(11)
    dev = lambda a: torch.from_numpy(a).cuda()
    rad = dev(np.concatenate([rng.uniform(0, 1, (S, 3)), rng.uniform(0, 4, (S, 1))], axis=1).astype(np.float32))
    steps = dev(rng.uniform(0.01, 0.05, S).astype(np.float32))
    num_hits = dev(np.asarray(hits, np.int32))
    indices = dev(np.concatenate([[0], np.cumsum(hits)[:-1]]).astype(np.int32))
    target = dev(rng.uniform(0, 1, (n, 3)).astype(np.float32))
    structs = _inactive(api)
    bg, loss, reg = (C.byref(structs[k]) for k in ("bg", "loss", "reg"))
    calls = [("rtxn_volrender_l2_train", []), ("rtxn_volrender_l2_train_ex", [None]), ("rtxn_volrender_l2_train_ex", [bg]),
             ("rtxn_volrender_loss_train", [None, None]), ("rtxn_volrender_loss_train", [bg, loss]),
             ("rtxn_volrender_reg_train", [None, None, None]), ("rtxn_volrender_reg_train", [bg, loss, reg]),
             ("rtxn_volrender_scaled_train", [None, None, None, None]), ("rtxn_volrender_scaled_train", [bg, loss, reg, None])]
    want = None
    for sym, rest in calls:
        pixels = torch.full((n, 3), -1.0, device="cuda")
        loss_grads = torch.full((n, 3), -1.0, dtype=torch.float16, device="cuda")
        dout = torch.full((S, 4), -1.0, dtype=torch.float16, device="cuda")
        loss_sum = torch.full((1,), -1.0, device="cuda")
        _lib.check(getattr(lib, sym)(rad.data_ptr(), steps.data_ptr(), num_hits.data_ptr(), indices.data_ptr(), n, K, target.data_ptr(), 128.0,
                                     pixels.data_ptr(), loss_grads.data_ptr(), loss_sum.data_ptr(), dout.data_ptr(), *rest, api._stream()), sym)
        torch.cuda.synchronize()
        got = dict(pixels=pixels, loss_gradients=loss_grads, radiance_gradients=dout, loss_sum=loss_sum)
        if want is None:
            assert float(loss_sum) > 0 and float(dout.float().abs().max()) > 0 and float((pixels[1:] - pixels[0]).abs().max()) > 0
            want = got
            continue
        for k in want:
            assert torch.equal(got[k], want[k]), f"{sym}({'inactive' if any(rest) else 'NULL'}), K = {K}: {k} differs"
