"""The dynamic loss scale and gradient-norm clipping on the GPU (include/rtxn.h, rtxn_loss_scaler): the statistics
kernel against numpy's float64 norm, the Adam kernels that read the multiplier from the device against the _opt ones, the
compositor that reads the scale from the device against the by-value one, a scale that never moves against the fixed-scale run on
all three stepping paths, backoff out of an overflow, growth across a change, clipping, resume, and "off is off".

Trainer shapes are those of test_gpu_optimizer.py: grid 16, sphere occupancy, 900-ray camera batches, hash 64 x 4 and frequency
128 x 2, deterministic mode."""
import faulthandler
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, B = 16, 900
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
MODELS = [("hash", 64, 4), ("freq", 128, 2)]
MAXB = 2048                    # RTXN_GRAD_STATS_MAX_BLOCKS: the row length of the partials


@pytest.fixture(autouse=True)
def _own_timeout():
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def within_one_ulp(got, want64):
    want = np.float32(want64)
    return abs(float(np.float32(got)) - float(want)) <= float(np.spacing(np.abs(want)))


def _scaler(torch, api, **kw):
    """(struct, its eight state words, the partials) on the device"""
    cfg = api.loss_scaler(**kw)
    state, ws = api.loss_scaler_state_tensor(cfg), api.loss_scaler_workspace()
    return api.loss_scaler(cfg.init_scale, cfg.growth, cfg.backoff, cfg.growth_interval, cfg.min_scale, cfg.max_scale, cfg.max_grad_norm,
                           state=state, partials=ws), state, ws


def _options(torch, api):
    factor = torch.zeros(1, device="cuda")
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    return api.optimizer_options(None, 0.0, True, factor, guard), factor, guard


def _view(torch, values, offset):
    """a device tensor holding `values` that starts `offset` elements into its allocation (offset 1: no 16-byte alignment)"""
    t = torch.from_numpy(values)
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    buf[offset:offset + t.numel()].copy_(t)
    return buf[offset:offset + t.numel()]


def _blocks(n, half):
    words = (n * (2 if half else 4) + 15) // 16
    return min(MAXB, (words + 1023) // 1024)


# ---- 1. the statistics kernel ---------------------------------------------------------------------------------------------------
_VALUES = {}


def _values(n, half):
    """a seeded normal times 1e3, made once and never written"""
    if (n, half) not in _VALUES:
        _VALUES[(n, half)] = (np.random.default_rng(n + half).standard_normal(n) * 1e3).astype(np.float16 if half else np.float32)
    return _VALUES[(n, half)]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n", [1, 63, 4099, 1_000_003])
def test_statistics_kernel_norm_flag_and_determinism(gpu, n, half, offset):
    """sqrt of the reduced sum, rounded to float, against numpy's float64 norm: within 1 ulp of float32 -- a double sum of 1e6
    terms is off by at most about 1e-10 relatively, far below a float ulp, and the one ulp covers the final rounding.  The sum is
    reduced twice: here (math.fsum over the partials) and by the scaler kernel (grad_norm at scale 1, divisor 1)."""
    torch = gpu
    from rtx_nerf_amd import api
    v = _values(n, half)
    g = _view(torch, v, offset)
    sc, state, ws = _scaler(torch, api, init_scale=1.0, min_scale=1.0)
    opt, _, guard = _options(torch, api)
    nb = _blocks(n, half)
    ws.fill_(-1.0)
    api.gradient_statistics([g], guard, sc)
    first = ws.clone()
    api.gradient_statistics([g], guard, sc)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int64), ws.view(torch.int64))                      # two launches: the same bits
    assert bool((ws[nb:] == -1.0).all()) and bool((ws[:nb] >= 0.0).all())                  # one double per block of this buffer, no other
    want = float(np.sqrt((v.astype(np.float64) ** 2).sum()))
    got = math.sqrt(math.fsum(ws[:nb].cpu().numpy().tolist()))
    step, rate = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    api.loss_scaler_step(opt, sc, [g], step, rate)
    dev_norm = float(state.view(torch.float32)[6].item())
    print(f"n={n} {'fp16' if half else 'fp32'} offset={offset}: blocks {nb}, norm {got!r} / device {dev_norm!r}, numpy float64 {want!r}")
    assert within_one_ulp(got, want) and within_one_ulp(dev_norm, want)
    assert int(guard[0].item()) == 0 and int(guard[1].item()) == 0 and int(state[2].item()) == 1     # nothing set the flag; a clean step
    # an Inf or a NaN at the first, the middle and the last element sets the flag
    for pos in sorted({0, n // 2, n - 1}):
        for bad in (float("inf"), float("nan")):
            keep = g[pos].clone()
            g[pos] = bad
            guard.zero_()
            api.gradient_statistics([g], guard, sc)
            assert int(guard[0].item()) == 1, (pos, bad)
            g[pos] = keep
    guard.zero_()
    api.gradient_statistics([g], guard, sc)
    assert int(guard[0].item()) == 0 and torch.equal(first.view(torch.int64)[:nb], ws.view(torch.int64)[:nb])


def test_statistics_of_four_buffers_in_one_launch_equal_the_four_singly(gpu):
    torch = gpu
    from rtx_nerf_amd import api
    spec = [(1_000_003, True, 1), (63, False, 0), (4099, True, 0), (1, False, 1)]
    bufs = [_view(torch, _values(n, half), off) for n, half, off in spec]
    sc, state, ws = _scaler(torch, api, init_scale=1.0)
    _, _, guard = _options(torch, api)
    api.gradient_statistics(bufs, guard, sc)
    joint = ws.clone()
    for k, (n, half, off) in enumerate(spec):
        ws.fill_(-1.0)
        api.gradient_statistics([bufs[k]], guard, sc)
        nb = _blocks(n, half)
        assert torch.equal(ws[:nb].view(torch.int64), joint[k * MAXB:k * MAXB + nb].view(torch.int64)), spec[k]
    assert int(guard[0].item()) == 0


# ---- 2. Adam reading the multiplier ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mult", [2.0 ** -7, 0.3 * 2.0 ** -7])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("sparse", [False, True])
def test_scaled_adam_is_the_opt_kernel_on_premultiplied_gradients(gpu, sparse, half, offset, mult):
    """n = 4099: a vector body and a scalar tail; offset 1: the scalar path alone.  The reference is the existing _opt entry point
    given fp32 gradients float32(g) * m with loss_scale = 1: the same product, then an exact factor of 1."""
    torch = gpu
    from rtx_nerf_amd import api
    n, lr = 4099, 1e-2
    rng = np.random.default_rng(11 + offset + 2 * half + 4 * sparse)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)).astype(np.float16 if half else np.float32)
    if sparse:
        g[rng.uniform(size=n) < 0.6] = 0                    # entries the sparse rule leaves alone
    m32 = np.float32(mult)
    master0 = rng.standard_normal(n).astype(np.float32)
    m0, v0 = (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.uniform(0, 1, n) * 0.01).astype(np.float32)
    steps0 = rng.integers(0, 5, n).astype(np.int32)
    sc, state, _ = _scaler(torch, api, init_scale=128.0)
    state.view(torch.float32)[1] = float(m32)
    opt, _, guard = _options(torch, api)
    step, rate = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    api.optimizer_rate(opt, step, rate, lr=lr)              # the rate, the factor and a clear skip word

    def run(scaled, skip=False):
        w, mm, vv = _view(torch, master0, offset), _view(torch, m0, offset), _view(torch, v0, offset)
        p16, st = _view(torch, master0.astype(np.float16), offset), _view(torch, steps0, offset)
        gd = _view(torch, g if scaled else g.astype(np.float32) * m32, offset)
        guard[2] = 1 if skip else 0
        if sparse and scaled:
            api.adam_step_sparse_scaled(w, p16, gd, mm, vv, st, opt, sc, lr=lr, eps=1e-15, zero_grads=True, weight_decay=False)
        elif sparse:
            api.adam_step_sparse_opt(w, p16, gd, mm, vv, st, opt, lr=lr, eps=1e-15, loss_scale=1.0, zero_grads=True, weight_decay=False)
        elif scaled:
            api.adam_step_scaled(w, p16, gd, mm, vv, rate, opt, sc, lr=lr, zero_grads=True)
        else:
            api.adam_step_opt(w, p16, gd, mm, vv, rate, opt, lr=lr, loss_scale=1.0, zero_grads=True)
        torch.cuda.synchronize()
        guard[2] = 0
        return dict(master=w, params=p16, m=mm, v=vv, steps=st, grads=gd)

    got, want = run(True), run(False)
    for k in ("master", "params", "m", "v", "steps"):
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["master"], torch.from_numpy(master0).cuda())                  # a step was taken
    assert int(got["grads"].count_nonzero().item()) == 0                                     # and the gradient consumed
    skipped = run(True, skip=True)                           # the skip word: the state keeps its bits, the gradient is cleared
    for k, ref in (("master", master0), ("params", master0.astype(np.float16)), ("m", m0), ("v", v0), ("steps", steps0)):
        assert torch.equal(skipped[k], torch.from_numpy(ref).cuda()), k
    assert int(skipped["grads"].count_nonzero().item()) == 0


# ---- 3. the compositor reading the scale ----------------------------------------------------------------------------------------
def _bits(t):
    """the raw words of a float tensor: Inf and NaN compare like any other bits"""
    import torch
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _deterministic(torch, api):
    """registers a fixed-point shadow: the compositor's loss scalar is then summed in a fixed order, the same bits every launch"""
    api.set_deterministic(api.deterministic_shadow(16), None)


def _loss_case(torch, api, K, case, kind, scale, scaler):
    """the loss compositor on one of test_gpu_train_loss.py's batches: by value (scaler None) or with the device word at `scale`"""
    import test_gpu_train_loss as T
    nh, idx, P, rad, step, tgt, bg_np = T.case_inputs(K, case)
    lam = 0.0 if case == "none3" else T.LAMBDA
    bg, _keep = T._bg_struct(torch, api, case)
    dev = T._to_dev(torch, rad=rad, step=step, nh=nh, idx=idx, tgt=tgt)
    n = T.B_RAYS
    out = dict(pix=torch.zeros((n, 3), device="cuda"), lg=torch.zeros((n, 3), dtype=torch.float16, device="cuda"),
               loss=torch.full((1,), 9.0, device="cuda"), grads=torch.zeros((P * K, 4), dtype=torch.float16, device="cuda"),
               opa=torch.full((n,), -1.0, device="cuda"))
    spec = api.train_loss(kind, opacity_weight=lam, opacity=out["opa"])
    a = (dev["rad"], dev["step"], dev["nh"], dev["idx"], n, K, dev["tgt"])
    b = (out["pix"], out["lg"], out["loss"], out["grads"], bg, spec)
    if scaler is None:
        api.volrender_loss_train(*a, scale, *b)
    else:
        scaler[1].view(torch.float32)[0] = scale
        api.volrender_scaled_train(*a, scaler[0], *b)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("case,kind", [("none3", "l1"), ("constant4", "huber"), ("random4", "relative_l2")])
def test_scaled_compositor_is_the_by_value_one_at_the_word_it_reads(gpu, case, kind, K):
    """pixels, opacities, fp16 loss gradients, radiance gradients and the loss sum (deterministic mode: a fixed-order sum), bit for
    bit, with the word at 128, 2^-3 and 2^15: the word is what is read"""
    torch = gpu
    from rtx_nerf_amd import api
    sc = _scaler(torch, api, init_scale=128.0, min_scale=2.0 ** -3, max_scale=2.0 ** 15)
    _deterministic(torch, api)
    try:
        seen = []
        for scale in (128.0, 2.0 ** -3, 2.0 ** 15):
            want, got = _loss_case(torch, api, K, case, kind, scale, None), _loss_case(torch, api, K, case, kind, scale, sc)
            for k in want:
                assert torch.equal(_bits(got[k]), _bits(want[k])), (k, scale)
            assert float(got["loss"].item()) != 9.0 and int(got["grads"].count_nonzero().item()) > 0
            seen.append(got)
        assert not torch.equal(_bits(seen[0]["lg"]), _bits(seen[1]["lg"])) and not torch.equal(_bits(seen[0]["lg"]), _bits(seen[2]["lg"]))
        assert torch.equal(seen[0]["pix"], seen[1]["pix"]) and torch.equal(seen[0]["loss"], seen[2]["loss"])      # the loss is unscaled
    finally:
        api.set_deterministic(None, None)


@pytest.mark.parametrize("K", [32, 7])
def test_scaled_regularised_compositor_is_the_by_value_one(gpu, K, monkeypatch):
    """REG once (Huber over a constant background with the alpha term, lambda_d = 10): k is formed in the kernel from the word by
    make_reg_args's expression; distortion and depth are compared as well"""
    torch = gpu
    from rtx_nerf_amd import api
    import test_gpu_distortion as D
    sc, state, _ = _scaler(torch, api, init_scale=128.0, min_scale=2.0 ** -3, max_scale=2.0 ** 15)
    by_value = api.volrender_reg_train
    _deterministic(torch, api)
    try:
        for scale in (128.0, 2.0 ** -3, 2.0 ** 15):
            monkeypatch.setattr(api, "volrender_reg_train", lambda *a, s=scale: by_value(*a[:7], s, *a[8:]))
            want = D._run(torch, api, K, "huber_constant4")

            def scaled(*a, s=scale):
                state.view(torch.float32)[0] = s
                api.volrender_scaled_train(*a[:7], sc, *a[8:])
            monkeypatch.setattr(api, "volrender_reg_train", scaled)
            got = D._run(torch, api, K, "huber_constant4")
            for k in want:
                assert got[k].tobytes() == want[k].tobytes(), (k, scale)
            assert got["dist"].max() > 0 and np.count_nonzero(got["out"]) > 0
    finally:
        api.set_deterministic(None, None)


@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("case", ["none3", "constant4", "random4"])
def test_l2_through_the_scaled_entry_against_float64_autograd(gpu, case, K, monkeypatch):
    """plain L2 runs the template here (it is one of loss_term's kinds): test_gpu_train_loss.py's float64 check of its kinds, at
    its tolerances, with the call routed through the scaled entry"""
    torch = gpu
    from rtx_nerf_amd import api
    import test_gpu_train_loss as T
    sc, state, _ = _scaler(torch, api, init_scale=T.LS)
    monkeypatch.setattr(api, "volrender_loss_train", lambda *a: api.volrender_scaled_train(*a[:7], sc, *a[8:]))
    T._check_compositor(torch, "l2", case, K)
    assert float(state.view(torch.float32)[0].item()) == T.LS


# ---- the trainers -----------------------------------------------------------------------------------------------------------------
def _occ(torch):
    from rtx_nerf_amd import scenes
    return torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()


def _trainer(torch, encoding, neurons, layers, **kw):
    from rtx_nerf_amd.train import Trainer
    kw.setdefault("deterministic", True)
    kw.setdefault("loss_scale", 128.0)
    return Trainer(R, _occ(torch), encoding=encoding, n_neurons=neurons, n_hidden_layers=layers, hashgrid=HGD if encoding == "hash" else None,
                   n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2, density_scale=120.0, mode="nerf", seed=3, **kw)


_BATCHES = {}


def _batch(torch, i=0):
    """camera batch i and its targets, made once and never written"""
    if i not in _BATCHES:
        from rtx_nerf_amd import scenes
        from rtx_nerf_amd.train import camera_rays
        o, d = camera_rays(scenes.pose_spherical(40.0 + 50.0 * i, -30.0 + 5.0 * i, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
        t = torch.from_numpy(np.random.default_rng(i).uniform(0, 1, (B, 3)).astype(np.float32)).cuda()
        _BATCHES[i] = (o, d, t)
    return _BATCHES[i]


def _state(tr):
    names = ["master", "params", "adam_m", "adam_v"] + (["table_master", "table", "table_m", "table_v", "table_steps"] if tr.encoding == "hash" else [])
    return {k: getattr(tr, k).clone() for k in names}


def _same(torch, a, b):
    """names of the state tensors that differ"""
    return [k for k in a if not torch.equal(a[k], b[k])]


def _grads(tr):
    return [tr.dparams] + ([tr.dtable] + ([tr.dtable_h] if tr.dtable_h is not None else []) if tr.encoding == "hash" else [])


PATHS = ("eager", "captured", "entry")


def _prepare(tr, path):
    if path == "captured":
        tr.capture_step(B, launch_segments=B * 30)
    elif path == "entry":
        tr.entry_args(B, launch_segments=B * 30)
    return tr


def _step(torch, tr, path, batch):
    o, d, t = batch
    if path == "eager":
        tr.step(o, d, t)
    else:
        tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
        tr.step_captured() if path == "captured" else tr.step_entry()
    torch.cuda.synchronize()


# ---- 4. a scale that never moves is the fixed run ---------------------------------------------------------------------------------
@pytest.mark.parametrize("distortion_weight", [0.0, 0.01])
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_a_scale_that_never_moves_is_the_fixed_scale_run_bit_for_bit(gpu, encoding, neurons, layers, distortion_weight):
    """Huber, so that both twins run the compositor template; powers of two are exact in fp32, so 1 / (128 D) is the same factor
    whether the host forms it or the scaler kernel does"""
    torch = gpu
    from rtx_nerf_amd import api
    kw = dict(loss="huber", distortion_weight=distortion_weight)
    trs = {}
    for p in PATHS:
        trs[("dynamic", p)] = _prepare(_trainer(torch, encoding, neurons, layers, loss_scale=api.loss_scaler(init_scale=128.0, growth_interval=10 ** 6),
                                                **kw), p)
        trs[("fixed", p)] = _prepare(_trainer(torch, encoding, neurons, layers, loss_scale=128.0, skip_nonfinite=True, **kw), p)
    start = _state(trs[("fixed", "eager")])
    for i in range(4):
        for (_, p), tr in trs.items():
            _step(torch, tr, p, _batch(torch, i))
    ref = _state(trs[("fixed", "eager")])
    assert len(_same(torch, start, ref)) == len(ref)                                        # four real steps
    for key, tr in trs.items():
        assert _same(torch, ref, _state(tr)) == [], key
        assert int(tr.skipped_steps.item()) == 0 and tr.step_count == 4
    for p in PATHS:
        tr = trs[("dynamic", p)]
        assert float(tr.loss_scale_now.item()) == 128.0 and int(tr.clipped_steps.item()) == 0 and int(tr._scaler_state[2].item()) == 4
        assert float(tr._scaler_state.view(torch.float32)[1].item()) == 1.0 / 128.0 and float(tr.grad_norm.item()) > 0.0
        assert trs[("fixed", p)].loss_scale_now is None


# ---- 5. backoff ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_backoff_out_of_an_overflow_on_every_path(gpu, encoding, neurons, layers):
    torch = gpu
    from rtx_nerf_amd import api
    batch = _batch(torch, 0)
    control = _trainer(torch, encoding, neurons, layers, loss_scale=2.0 ** 40, skip_nonfinite=True)
    before = _state(control)
    control.step(*batch)
    torch.cuda.synchronize()
    assert int(control.skipped_steps.item()) == 1 and _same(torch, before, _state(control)) == []      # what guarantees the overflow
    finals, ks = {}, {}
    for p in PATHS:
        tr = _prepare(_trainer(torch, encoding, neurons, layers,
                               loss_scale=api.loss_scaler(init_scale=2.0 ** 40, max_scale=2.0 ** 40, backoff=2.0 ** -4)), p)
        start, k = _state(tr), 0
        while True:
            assert float(tr.loss_scale_now.item()) == 2.0 ** (40 - 4 * k)                   # exactly 2^40, 2^36, ...
            _step(torch, tr, p, batch)
            if int(tr.skipped_steps.item()) == k:                                            # a finite step
                break
            k += 1
            assert k <= 10 and int(tr.skipped_steps.item()) == k and int(tr.scale_backoffs.item()) == k
            assert _same(torch, start, _state(tr)) == []                                     # the state is untouched ...
            assert all(int(g.count_nonzero().item()) == 0 for g in _grads(tr))               # ... and the gradients are cleared
        assert 1 <= k <= 10
        assert int(tr.scale_backoffs.item()) == int(tr.skipped_steps.item()) == k and tr.step_count == k + 1
        assert float(tr.loss_scale_now.item()) == 2.0 ** (40 - 4 * k) and len(_same(torch, start, _state(tr))) == len(start)
        assert all(bool(torch.isfinite(v.float()).all()) for v in _state(tr).values())
        finals[p], ks[p] = _state(tr), k
        print(f"{encoding} {p}: {k} steps skipped, the first finite step at scale 2^{40 - 4 * k}")
    assert ks["eager"] == ks["captured"] == ks["entry"]
    for p in PATHS[1:]:
        assert _same(torch, finals["eager"], finals[p]) == [], p


# ---- 6. growth across a change -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_growth_across_a_change_agrees_with_fixed_scale_steps(gpu, encoding, neurons, layers, tmp_path):
    torch = gpu
    from rtx_nerf_amd import api
    tr = _trainer(torch, encoding, neurons, layers, loss="huber", loss_scale=api.loss_scaler(init_scale=16.0, growth_interval=2))
    fixed = {}
    scales = []
    for i in range(6):
        s = float(tr.loss_scale_now.item())
        scales.append(s)
        if 1 <= i <= 3:                                       # steps 2 to 4: the same step from the same state at the scale in force
            path = str(tmp_path / f"before_{i}.ckpt")
            tr.save_checkpoint(path)
            if s not in fixed:
                fixed[s] = _trainer(torch, encoding, neurons, layers, loss="huber", loss_scale=s, skip_nonfinite=True)
            fixed[s].load_checkpoint(path)
            fixed[s].step(*_batch(torch, i))
        tr.step(*_batch(torch, i))
        torch.cuda.synchronize()
        if 1 <= i <= 3:
            assert _same(torch, _state(tr), _state(fixed[s])) == [], (i, s)
            assert int(fixed[s].skipped_steps.item()) == 0 and fixed[s].step_count == tr.step_count == i + 1
    assert scales == [16.0, 16.0, 32.0, 32.0, 64.0, 64.0] and sorted(fixed) == [16.0, 32.0]
    assert float(tr.loss_scale_now.item()) == 128.0 and int(tr.scale_growths.item()) == 3 and int(tr.skipped_steps.item()) == 0


# ---- 7. clipping -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_clipping_is_the_opt_kernels_on_gradients_times_the_device_multiplier(gpu, encoding, neurons, layers):
    torch = gpu
    from rtx_nerf_amd import api
    batch = _batch(torch, 0)
    never = dict(init_scale=128.0, growth_interval=10 ** 6)
    twin = _trainer(torch, encoding, neurons, layers, loss_scale=api.loss_scaler(**never))
    start = _state(twin)
    assert twin.gradients(*batch) > 0
    g_mlp = twin.dparams.clone()
    g_tab = twin.table_grad() if encoding == "hash" else None
    parts = []                                               # (slice of the table, its gradient as the optimizer consumes it)
    if encoding == "hash":
        lo = twin.hashed_lo
        parts = [(slice(0, lo), twin.dtable[:lo].clone()), (slice(lo, None), twin.dtable_h.clone())] if twin.hash_fp16 else [(slice(None), twin.dtable.clone())]
    twin.apply_gradients(1.0)
    torch.cuda.synchronize()
    norm = float(twin.grad_norm.item())
    sq = float((g_mlp.double() ** 2).sum().item()) + (float((g_tab.double() ** 2).sum().item()) if g_tab is not None else 0.0)
    want = math.sqrt(sq) / 128.0
    print(f"{encoding}: grad_norm {norm!r}, float64 {want!r}")
    assert norm > 0.0 and within_one_ulp(norm, want) and int(twin.clipped_steps.item()) == 0

    clipped = _trainer(torch, encoding, neurons, layers, loss_scale=api.loss_scaler(**never), max_grad_norm=norm / 2)
    clipped.step(*batch)
    torch.cuda.synchronize()
    assert int(clipped.clipped_steps.item()) == 1 and float(clipped.grad_norm.item()) == norm and int(clipped.skipped_steps.item()) == 0
    mult = clipped._scaler_state.view(torch.float32)[1:2].clone()
    f = np.float32
    coef = f(f(norm / 2) / f(f(norm) + f(1e-6)))            # max_grad_norm / (norm + 1e-6), below 1
    assert coef < 1 and f(mult.item()).tobytes() == f(coef * f(f(1) / f(128))).tobytes()
    # by hand: the existing _opt kernels on a fresh trainer's state, the twin's gradients pre-multiplied in fp32, loss_scale 1
    hand = _trainer(torch, encoding, neurons, layers, loss_scale=128.0, skip_nonfinite=True)
    assert _same(torch, start, _state(hand)) == []
    step, rates = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    api.optimizer_rate(hand._opt, step, rates[0:1], lr=hand.lr, table_lr=hand.lr * 10.0, table_effective_lr=rates[1:2])
    api.adam_step_opt(hand.master, hand.params, g_mlp * mult, hand.adam_m, hand.adam_v, rates[0:1], hand._opt, lr=hand.lr, loss_scale=1.0)
    for sl, g in parts:
        if g.numel():
            api.adam_step_sparse_opt(hand.table_master[sl], hand.table[sl], g.float() * mult, hand.table_m[sl], hand.table_v[sl],
                                     hand.table_steps[sl], hand._opt, lr=hand.lr * 10.0, eps=1e-15, loss_scale=1.0, weight_decay=False)
    torch.cuda.synchronize()
    assert _same(torch, _state(clipped), _state(hand)) == []
    assert len(_same(torch, _state(clipped), _state(twin))) > 0

    loose = _trainer(torch, encoding, neurons, layers, loss_scale=api.loss_scaler(**never), max_grad_norm=norm * 2)
    loose.step(*batch)
    torch.cuda.synchronize()
    assert int(loose.clipped_steps.item()) == 0 and _same(torch, _state(loose), _state(twin)) == []

    fixed = _trainer(torch, encoding, neurons, layers, loss_scale=128.0, max_grad_norm=norm / 2)          # a fixed scale, clipping only
    fixed.step(*batch)
    torch.cuda.synchronize()
    assert int(fixed.clipped_steps.item()) == 1 and _same(torch, _state(fixed), _state(clipped)) == []


# ---- 8. resume -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_resume_continues_the_scalers_sequence(gpu, encoding, neurons, layers, tmp_path):
    torch = gpu
    from rtx_nerf_amd import api
    make = lambda: _trainer(torch, encoding, neurons, layers, loss_scale=api.loss_scaler(init_scale=16.0, growth_interval=3), max_grad_norm=1e3)
    straight = make()
    for i in range(6):
        straight.step(*_batch(torch, i))
    first = make()
    for i in range(4):
        first.step(*_batch(torch, i))
    path = str(tmp_path / "four.ckpt")
    first.save_checkpoint(path)
    assert float(first.loss_scale_now.item()) == 32.0 and int(first._scaler_state[2].item()) == 1      # one growth behind, one clean step since
    second = make()
    header = second.load_checkpoint(path)
    assert header["loss_scaler"]["scale"] == 32.0 and header["loss_scaler"]["good"] == 1 and header["loss_scaler"]["growths"] == 1
    assert torch.equal(second._scaler_state, first._scaler_state)
    for i in range(4, 6):
        second.step(*_batch(torch, i))
    torch.cuda.synchronize()
    assert _same(torch, _state(straight), _state(second)) == []
    assert torch.equal(straight._scaler_state, second._scaler_state)
    assert float(second.loss_scale_now.item()) == 64.0 and int(second.scale_growths.item()) == 2 and second.step_count == 6
    plain = _trainer(torch, encoding, neurons, layers)         # a trainer without a scaler reads the same file
    plain.load_checkpoint(path)
    assert _same(torch, _state(plain), _state(first)) == [] and plain.loss_scale_now is None and plain.step_count == 4


# ---- 9. off is off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_off_is_off(gpu, encoding, neurons, layers):
    torch = gpu
    from rtx_nerf_amd.train import Trainer
    without = Trainer(R, _occ(torch), encoding=encoding, n_neurons=neurons, n_hidden_layers=layers, hashgrid=HGD if encoding == "hash" else None,
                      n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2, density_scale=120.0, mode="nerf", seed=3, deterministic=True)
    defaults = _trainer(torch, encoding, neurons, layers, loss_scale=128.0, max_grad_norm=None)
    for tr in (without, defaults):
        assert tr._scaler is None and tr._scaler_state is None and tr._scaler_ws is None and tr._opt is None and tr._opt_guard is None
        assert tr.loss_scale_now is None and tr.grad_norm is None and tr.clipped_steps is None and tr.skipped_steps is None
        assert tr.loss_scale == 128.0
    for i in range(3):
        without.step(*_batch(torch, i))
        defaults.step(*_batch(torch, i))
    torch.cuda.synchronize()
    assert _same(torch, _state(without), _state(defaults)) == []
