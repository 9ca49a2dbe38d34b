"""The optimizer options on the GPU (include/rtxn.h, rtxn_optimizer_options): the _opt Adam kernels against the
oracle's fp32 Adam with the scheduled rate and the decay term applied in numpy, the skip word, the gradient check kernel, the rate
kernel against the host functions, the three stepping paths against each other bit for bit, "off is off", the non-finite guard on
every path, and resume / the schedule past the captured step's bias-correction table.

Trainer shapes are those of test_gpu_sample_jitter.py: grid 16, sphere occupancy, 30 x 30 camera batches, hash 64 x 4 and
frequency 128 x 2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, B = 16, 900
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
MODELS = [("hash", 64, 4), ("freq", 128, 2)]
# warm-up over two steps, then x0.5 per two steps from step 3 on: factor 0.5, 1, 0.707, 0.5, 0.354 over five steps
SCHED = dict(kind="exponential", warmup_steps=2, decay_start=2, decay_steps=2, ratio=0.5)
WARMUP, START, STEPS = 40, 100, 600
T_LIST = [1, WARMUP - 1, WARMUP, WARMUP + 1, START, START + 1, START + STEPS // 2, START + STEPS, START + STEPS + 1, 70_000]


def factor64(t, kind="constant", warmup_steps=0, decay_start=0, decay_steps=1, ratio=1.0, staircase=False):
    """include/rtxn.h's factor(t) in float64; the ratio is the float32 the struct holds"""
    warm = min(1.0, t / warmup_steps) if warmup_steps > 0 else 1.0
    x = max(0, t - decay_start) / decay_steps
    if staircase:
        x = np.floor(x)
    r = float(np.float32(ratio))
    dec = 1.0 if kind == "constant" else r ** x if kind == "exponential" else r + (1.0 - r) * (1.0 + np.cos(np.pi * min(x, 1.0))) / 2.0
    return warm * dec


def ulps(got, want):
    want = np.float32(want)
    return abs(float(np.float32(got)) - float(want)) / float(np.spacing(np.abs(want)))


def _occ(torch):
    from rtx_nerf_amd import scenes
    return torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()


def _trainer(torch, encoding, neurons, layers, **kw):
    from rtx_nerf_amd.train import Trainer
    kw.setdefault("deterministic", True)
    return Trainer(R, _occ(torch), encoding=encoding, n_neurons=neurons, n_hidden_layers=layers, hashgrid=HGD if encoding == "hash" else None,
                   n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2, loss_scale=128.0, density_scale=120.0, mode="nerf", seed=3, **kw)


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


def _finite(torch, st):
    return all(bool(torch.isfinite(v.float()).all()) for v in st.values())


def _grads(tr):
    return [tr.dparams] + ([tr.dtable] + ([tr.dtable_h] if tr.dtable_h is not None else []) if tr.encoding == "hash" else [])


class _Paths:
    """one trainer behind each of the three stepping methods"""

    def __init__(self, torch, encoding, neurons, layers, which=("eager", "captured", "entry"), **kw):
        self.torch = torch
        self.tr = {p: _trainer(torch, encoding, neurons, layers, **kw) for p in which}
        if "captured" in self.tr:
            self.tr["captured"].capture_step(B, launch_segments=B * 30)
        if "entry" in self.tr:
            self.tr["entry"].entry_args(B, launch_segments=B * 30)

    def step(self, o, d, t):
        for p, tr in self.tr.items():
            if p == "eager":
                tr.step(o, d, t)
            else:
                tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
                tr.step_captured() if p == "captured" else tr.step_entry()
        self.torch.cuda.synchronize()


# ---- 1. Adam variants against the fp32 restatement ------------------------------------------------------------------------------
def _options(torch, api, sched=None, weight_decay=0.0, skip_nonfinite=False):
    factor = torch.zeros(1, device="cuda")
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    return api.optimizer_options(sched, weight_decay, skip_nonfinite, factor, guard), factor, guard


def _views(torch, n, offset, *dtypes):
    """zeroed tensors of n elements that start `offset` elements into their allocation (offset 1: no 16-byte alignment)"""
    return [torch.zeros(n + 8, dtype=dt, device="cuda")[offset:offset + n] for dt in dtypes]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("half_grads", [False, True])
def test_dense_adam_opt_matches_the_oracle_with_the_scheduled_rate_and_decay(gpu, oracle, half_grads, offset):
    """rtxn_adam_step_opt over five steps: the rate kernel's bias-corrected rate of lr factor(t), then w -= lr_t wd w.  n = 10 003:
    a vector body and a scalar tail; offset 1: the scalar path alone.  Reference: oracle.adam_step with lr factor, the decay term
    in numpy float32.  Tolerances: tests/test_gpu_train.py's for adam_kernel."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(7 + offset)
    n, lr, wd, ls = 10_003, 1e-2, 0.1, 4.0
    sched = dict(kind="exponential", decay_steps=4, ratio=0.5)
    opt, factor_d, _ = _options(torch, api, sched, wd)
    md, mm, vv, p16d = _views(torch, n, offset, torch.float32, torch.float32, torch.float32, torch.float16)
    gd, = _views(torch, n, offset, torch.float16 if half_grads else torch.float32)
    master = rng.standard_normal(n).astype(np.float32)
    md.copy_(torch.from_numpy(master))
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    step_d, rate_d = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    for t in range(1, 6):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 1, n)).astype(np.float16 if half_grads else np.float32)
        gd.copy_(torch.from_numpy(g))
        api.optimizer_rate(opt, step_d, rate_d, lr=lr)
        api.adam_step_opt(md, p16d, gd, mm, vv, rate_d, opt, lr=lr, loss_scale=ls, zero_grads=(t % 2 == 1))
        f = np.float32(factor_d.item())
        assert int(step_d.item()) == t and f != 1.0 and ulps(f, factor64(t, **sched)) <= 1
        lr_t = np.float32(lr) * f
        oracle.adam_step(master, g.astype(np.float32), m, v, t, lr=float(lr_t), loss_scale=ls)
        master -= (lr_t * np.float32(wd)) * master
        left = gd.cpu().numpy()
        assert (not left.any()) if t % 2 == 1 else np.array_equal(left, g)
    np.testing.assert_allclose(md.cpu().numpy(), master, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(mm.cpu().numpy(), m, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(vv.cpu().numpy(), v, rtol=1e-6, atol=1e-12)
    same = (p16d.cpu().numpy() == master.astype(np.float16)).mean()
    print(f"fp16 parameters equal to the rounded reference master: {same:.6f}")
    assert same > 0.9999


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("half_grads", [False, True])
def test_sparse_adam_opt_matches_the_oracle_with_the_scheduled_rate_and_decay(gpu, oracle, half_grads, offset):
    """rtxn_adam_step_sparse_opt as test_adam_sparse_matches_oracle drives rtxn_adam_step_sparse: five steps of gradients that are
    zero on a different 90 % of the entries, whole 4-groups and waves among them; lr factor(t) in the entry's own bias correction
    and the decay term on the entries the step updates."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(11 + offset)
    n, lr, wd, ls = 10_003, 1e-2, 0.1, 4.0
    sched = dict(kind="exponential", decay_steps=4, ratio=0.5)
    opt, factor_d, _ = _options(torch, api, sched, wd)
    md, mm, vv, p16d, sd = _views(torch, n, offset, torch.float32, torch.float32, torch.float32, torch.float16, torch.int32)
    gd, = _views(torch, n, offset, torch.float16 if half_grads else torch.float32)
    master = rng.standard_normal(n).astype(np.float32) * 1e-2
    md.copy_(torch.from_numpy(master))
    start = master.copy()
    m, v, st = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    never = np.ones(n, bool)
    step_d, rate_d = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    for t in range(1, 6):
        g = (rng.standard_normal(n) * 0.3).astype(np.float16 if half_grads else np.float32)
        g[rng.uniform(size=n) < 0.9] = 0
        if t == 3:
            g[:64] = 0                                    # whole 4-parameter groups and waves without a gradient
        never &= g == 0
        gd.copy_(torch.from_numpy(g))
        api.optimizer_rate(opt, step_d, rate_d, lr=lr)
        api.adam_step_sparse_opt(md, p16d, gd, mm, vv, sd, opt, lr=lr, eps=1e-15, loss_scale=ls, zero_grads=(t % 2 == 1))
        f = np.float32(factor_d.item())
        assert f != 1.0 and ulps(f, factor64(t, **sched)) <= 1
        lr_t = np.float32(lr) * f
        oracle.adam_step_sparse(master, g.astype(np.float32), m, v, st, lr=float(lr_t), eps=1e-15, loss_scale=ls)
        hit = g != 0
        master[hit] -= (lr_t * np.float32(wd)) * master[hit]
        np.testing.assert_array_equal(sd.cpu().numpy().view(np.uint32), st)
        np.testing.assert_allclose(md.cpu().numpy(), master, rtol=0, atol=3e-7)
        np.testing.assert_allclose(mm.cpu().numpy(), m, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(vv.cpu().numpy(), v, rtol=1e-6, atol=1e-12)
        left = gd.cpu().numpy()
        assert (not left.any()) if t % 2 == 1 else np.array_equal(left, g)
        touched = st > 0
        np.testing.assert_array_equal(p16d.cpu().numpy()[touched], md.cpu().numpy()[touched].astype(np.float16))
    assert never.any() and np.array_equal(md.cpu().numpy()[never], start[never]) and not st[never].any()


def test_no_weight_decay_flag_and_unit_factor_are_the_plain_kernels(gpu):
    """weight_decay=False (the hash table's calls) with a factor of exactly 1 (a one-step warm-up): the _opt kernels end on the
    bits of rtxn_adam_step_captured / rtxn_adam_step_sparse."""
    torch = gpu
    from rtx_nerf_amd import api
    n = 4_099
    opt, factor_d, _ = _options(torch, api, dict(warmup_steps=1), 0.3)
    g0 = torch.Generator().manual_seed(2)
    w0 = torch.randn(n, generator=g0).cuda()
    grad = (torch.randn(n, generator=g0) * (torch.rand(n, generator=g0) < 0.3)).cuda()
    step_d, rate_d = torch.full((1,), 6, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    api.optimizer_rate(opt, step_d, rate_d, lr=1e-2)
    assert float(factor_d.item()) == 1.0
    out = []
    for use_opt in (True, False):
        w, m, v, p = w0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.float16, device="cuda")
        ws, ms, vs, ps, ss = w0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.float16, device="cuda"), \
            torch.zeros(n, dtype=torch.int32, device="cuda")
        if use_opt:
            api.adam_step_opt(w, p, grad.clone(), m, v, rate_d, opt, lr=1e-2, loss_scale=2.0, weight_decay=False)
            api.adam_step_sparse_opt(ws, ps, grad.clone(), ms, vs, ss, opt, lr=1e-2, eps=1e-15, loss_scale=2.0, weight_decay=False)
        else:
            api.adam_step_captured(w, p, grad.clone(), m, v, rate_d, loss_scale=2.0)
            api.adam_step_sparse(ws, ps, grad.clone(), ms, vs, ss, lr=1e-2, eps=1e-15, loss_scale=2.0)
        out.append((w, m, v, p, ws, ms, vs, ps, ss))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][0], w0)


# ---- 2. the skip word --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("half_grads", [False, True])
def test_skip_word_leaves_the_state_and_clears_the_gradient(gpu, half_grads, offset):
    torch = gpu
    from rtx_nerf_amd import api
    n = 10_003
    opt, factor_d, guard = _options(torch, api, dict(warmup_steps=3), 0.1, skip_nonfinite=True)
    gen = torch.Generator().manual_seed(9)
    w, m, v, p, s = _views(torch, n, offset, torch.float32, torch.float32, torch.float32, torch.float16, torch.int32)
    gd, = _views(torch, n, offset, torch.float16 if half_grads else torch.float32)
    w.copy_(torch.randn(n, generator=gen)); m.copy_(torch.randn(n, generator=gen) * 0.1); v.copy_(torch.rand(n, generator=gen) * 0.1)
    p.copy_(w.half()); s.copy_(torch.randint(0, 9, (n,), generator=gen).int())
    grad = torch.randn(n, generator=gen)
    grad[::7] = float("nan"); grad[3] = float("inf"); grad[5::11] = 0.0
    step_d, rate_d = torch.full((1,), 4, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    guard[0] = 1                                            # what the check kernel leaves behind a bad gradient
    api.optimizer_rate(opt, step_d, rate_d, lr=1e-2)
    assert guard.tolist() == [0, 1, 1, 0] and int(step_d.item()) == 5
    before = [x.clone() for x in (w, m, v, p, s)]
    for sparse in (False, True):
        for zero in (False, True):
            gd.copy_(grad.to(gd.dtype))
            kept = gd.clone()
            if sparse:
                api.adam_step_sparse_opt(w, p, gd, m, v, s, opt, lr=1e-2, eps=1e-15, loss_scale=2.0, zero_grads=zero)
            else:
                api.adam_step_opt(w, p, gd, m, v, rate_d, opt, lr=1e-2, loss_scale=2.0, zero_grads=zero)
            torch.cuda.synchronize()
            for x, y in zip((w, m, v, p, s), before):
                assert torch.equal(x, y), (sparse, zero)
            if zero:
                assert not bool((gd.view(torch.int16 if half_grads else torch.int32) != 0).any()), (sparse, zero)
            else:
                assert torch.equal(gd.view(torch.int16 if half_grads else torch.int32), kept.view(torch.int16 if half_grads else torch.int32))
    # the next rate launch finds the flag clear: the skip word drops, the count stays, and the same call now updates
    api.optimizer_rate(opt, step_d, rate_d, lr=1e-2)
    assert guard.tolist() == [0, 1, 0, 0]
    gd.copy_(torch.randn(n, generator=gen).to(gd.dtype))
    api.adam_step_opt(w, p, gd, m, v, rate_d, opt, lr=1e-2, loss_scale=2.0)
    assert not torch.equal(w, before[0]) and bool(torch.isfinite(w).all())


# ---- 3. the check kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n", [1, 63, 4_099, 1_000_003])
def test_check_gradients_finds_every_nonfinite_element_and_nothing_else(gpu, n, half):
    """clean buffers (denormals, -0, +-65504 and the largest finite values among them) leave the flag clear; one Inf, -Inf or NaN
    in the first, the last or the first element behind the last whole 16 bytes sets it -- on an aligned buffer and on one that
    starts one element off a 16-byte boundary"""
    torch = gpu
    from rtx_nerf_amd import api
    dt = torch.float16 if half else torch.float32
    esize = 2 if half else 4
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    gen = torch.Generator().manual_seed(n)
    clean = torch.randn(n, generator=gen).to(dt)
    special = [65504.0, -65504.0, -0.0, 6e-8 if half else 1e-40, -(6e-8 if half else 1e-40), 0.0] + ([] if half else [3.4e38, -3.4e38])
    for k, x in enumerate(special):
        clean[(k * 9) % n] = x
    assert bool(torch.isfinite(clean).all())
    for offset in (0, 1):
        buf = torch.zeros(n + 8, dtype=dt, device="cuda")[offset:offset + n]
        buf.copy_(clean)
        api.check_gradients([buf], flag)
        assert flag.tolist() == [0, 0, 0, 0], f"clean buffer flagged (offset {offset})"
        head = min(n, ((16 - buf.data_ptr() % 16) % 16) // esize)
        tail = head + (n - head) // (16 // esize) * (16 // esize)
        assert (head > 0) == (offset == 1)
        places = sorted({0, n - 1, min(tail, n - 1), head if head < n else 0})
        for bad in (float("inf"), float("-inf"), float("nan")):
            for i in places:
                keep = buf[i].clone()
                buf[i] = bad
                api.check_gradients([buf], flag)
                assert flag.tolist() == [1, 0, 0, 0], f"{bad} at {i} of {n} not found (offset {offset})"
                flag.zero_()
                buf[i] = keep
        api.check_gradients([buf], flag)
        assert flag.tolist() == [0, 0, 0, 0]


def test_check_gradients_covers_every_buffer_of_one_launch(gpu):
    torch = gpu
    from rtx_nerf_amd import api
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    bufs = [torch.ones(5_001, device="cuda"), None, torch.ones(0, device="cuda"), torch.ones(777, dtype=torch.float16, device="cuda"),
            torch.ones(70_001, device="cuda"), torch.ones(33, dtype=torch.float16, device="cuda")]
    api.check_gradients(bufs, flag)
    assert flag.tolist() == [0, 0, 0, 0]
    for k in (0, 3, 4, 5):
        bufs[k][-2] = float("nan")
        api.check_gradients(bufs, flag)
        assert flag.tolist() == [1, 0, 0, 0], k
        flag.zero_()
        bufs[k][-2] = 1.0
    api.check_gradients([], flag)
    assert flag.tolist() == [0, 0, 0, 0]


# ---- 4. the rate kernel -----------------------------------------------------------------------------------------------------------
RATE_SCHEDULES = [dict(kind="constant", warmup_steps=WARMUP), dict(kind="exponential", warmup_steps=WARMUP, decay_start=START, decay_steps=STEPS, ratio=0.1),
                  dict(kind="exponential", warmup_steps=WARMUP, decay_start=START, decay_steps=STEPS, ratio=0.33, staircase=True),
                  dict(kind="exponential", decay_steps=250000, ratio=0.1), dict(kind="cosine", warmup_steps=WARMUP, decay_start=START, decay_steps=STEPS, ratio=0.1)]


@pytest.mark.parametrize("sched", RATE_SCHEDULES)
def test_rate_kernel_matches_the_host_functions(gpu, sched):
    """factor(t) and the MLP's and the table's bias-corrected rates from one launch per t over a device counter set with fill_,
    against rtxn_lr_schedule_factor and rtxn_adam_effective_lr(lr factor): 1 ulp."""
    torch = gpu
    from rtx_nerf_amd import api
    opt, factor_d, guard = _options(torch, api, sched)
    step_d, rates = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    lr, tlr = 1e-3, 1e-2
    for t in T_LIST:
        step_d.fill_(t - 1)
        api.optimizer_rate(opt, step_d, rates[0:1], lr=lr, table_lr=tlr, table_effective_lr=rates[1:2])
        f, (e, et) = float(factor_d.item()), rates.tolist()
        assert int(step_d.item()) == t
        fh = api.lr_schedule_factor(sched, t)
        eh = api.adam_effective_lr(float(np.float32(lr) * np.float32(fh)), 0.9, 0.999, t)
        eth = api.adam_effective_lr(float(np.float32(tlr) * np.float32(fh)), 0.9, 0.999, t)
        print(f"t={t}: factor {f!r} host {fh!r} float64 {factor64(t, **sched)!r}; rate {e!r} host {eh!r}; table {et!r} host {eth!r}")
        assert ulps(f, fh) <= 1 and ulps(f, factor64(t, **sched)) <= 1
        assert ulps(e, eh) <= 1 and ulps(et, eth) <= 1
        # advance = 0 reads the counter as it stands and gives the same values
        api.optimizer_rate(opt, step_d, rates[0:1], lr=lr, table_lr=tlr, table_effective_lr=rates[1:2], advance=False)
        assert int(step_d.item()) == t and float(factor_d.item()) == f and rates.tolist() == [e, et]
    assert guard.tolist() == [0, 0, 0, 0]


# ---- 5. three paths, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_three_paths_agree_bit_for_bit_under_schedule_and_decay(gpu, encoding, neurons, layers):
    torch = gpu
    P = _Paths(torch, encoding, neurons, layers, lr_schedule=SCHED, weight_decay=0.01)
    plain = _trainer(torch, encoding, neurons, layers)
    for i in range(5):
        P.step(*_batch(torch, i % 3))
        plain.step(*_batch(torch, i % 3))
        a = P.tr["eager"]
        for p in ("captured", "entry"):
            x = P.tr[p]
            assert torch.equal(a.params, x.params) and torch.equal(a.master, x.master), f"eager vs {p}, step {i}"
            if encoding == "hash":
                assert torch.equal(a.table_master, x.table_master), f"eager vs {p}, table, step {i}"
            assert _same(torch, _state(a), _state(x)) == []
        assert ulps(a._opt_factor.item(), factor64(i + 1, **SCHED)) <= 1
    assert all(tr.step_count == 5 for tr in P.tr.values())
    assert not torch.equal(plain.master, a.master) and not torch.equal(plain.params, a.params)
    assert _finite(torch, _state(a))


# ---- 6. off is off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_options_off_are_the_trainer_without_the_arguments(gpu, encoding, neurons, layers):
    torch = gpu
    base = _Paths(torch, encoding, neurons, layers)
    none = _Paths(torch, encoding, neurons, layers, lr_schedule=None, weight_decay=0.0, skip_nonfinite=False)
    const = _Paths(torch, encoding, neurons, layers, lr_schedule=dict(kind="constant"), weight_decay=0.0, skip_nonfinite=False)
    for tr in list(none.tr.values()) + list(const.tr.values()):
        assert tr._opt is None and tr._opt_guard is None and tr._opt_step is None and tr._opt_lr is None and tr.skipped_steps is None
        assert not hasattr(tr, "_opt_factor") and tr.current_lr() == float(np.float32(1e-2))
    for i in range(3):
        for P in (base, none, const):
            P.step(*_batch(torch, i))
        for p in ("eager", "captured", "entry"):
            for other in (none, const):
                assert _same(torch, _state(base.tr[p]), _state(other.tr[p])) == [], f"{p}, step {i}"


@pytest.mark.parametrize("env", [{}, {"RTXN_TABLE_ADAM": "dense"}, {"RTXN_HASH_GRAD_FP16": "0"}, {"RTXN_TABLE_ADAM": "dense", "RTXN_HASH_GRAD_FP16": "0"}])
def test_active_options_with_a_unit_factor_are_the_plain_optimizer(gpu, monkeypatch, env):
    """A one-step warm-up is an ACTIVE schedule whose factor is exactly 1 from the first update on: the step then runs the rate
    kernel and the _opt Adam kernels -- with RTXN_TABLE_ADAM=dense the dense kernel and the table's own bias-corrected rate, with
    RTXN_HASH_GRAD_FP16=0 one fp32 table gradient -- and must end on the plain trainer's bits (the rate kernel's double powers
    round to the host's powf for these t, trainer.hip)."""
    torch = gpu
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    which = ("eager", "captured") if "RTXN_TABLE_ADAM" in env else ("eager", "captured", "entry")
    plain = _Paths(torch, "hash", 64, 4, which=which)
    unit = _Paths(torch, "hash", 64, 4, which=which, lr_schedule=dict(warmup_steps=1), skip_nonfinite=True)
    assert plain.tr["eager"].table_adam_sparse == ("RTXN_TABLE_ADAM" not in env) and plain.tr["eager"].hash_fp16 == ("RTXN_HASH_GRAD_FP16" not in env)
    for i in range(3):
        plain.step(*_batch(torch, i))
        unit.step(*_batch(torch, i))
        for p in which:
            assert unit.tr[p]._opt is not None and _same(torch, _state(plain.tr[p]), _state(unit.tr[p])) == [], f"{p}, step {i}"
            assert int(unit.tr[p].skipped_steps.item()) == 0


# ---- 7. the guard ----------------------------------------------------------------------------------------------------------------
def _poisoned(torch, i=0):
    o, d, t = _batch(torch, i)
    t = t.clone()
    t[:, 0] = float("inf")              # targets feed only the loss: arithmetic, never an index
    return o, d, t


@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_guard_skips_a_nonfinite_step_on_every_path(gpu, encoding, neurons, layers):
    torch = gpu
    G = _Paths(torch, encoding, neurons, layers, skip_nonfinite=True)
    U = _Paths(torch, encoding, neurons, layers)                       # the unguarded twins: the control that the input poisons
    before = {p: _state(tr) for p, tr in G.tr.items()}
    G.step(*_poisoned(torch))
    U.step(*_poisoned(torch))
    for p, tr in G.tr.items():
        assert _same(torch, before[p], _state(tr)) == [], f"{p}: the skipped step moved the state"
        assert all(not bool((g != 0).any()) for g in _grads(tr)), f"{p}: gradients left behind"
        assert int(tr.skipped_steps.item()) == 1 and tr.step_count == 1, p
        assert not bool(torch.isfinite(U.tr[p].master).all()), f"{p}: the Inf target did not poison the unguarded twin"
    # injected straight into the gradient buffers the eager optimizer is about to consume
    injected = [("dparams", float("inf"))] + ([("dtable_h" if G.tr["eager"].hash_fp16 else "dtable", float("nan"))] if encoding == "hash" else [])
    twins = []
    for name, bad in injected:
        e = _trainer(torch, encoding, neurons, layers, skip_nonfinite=True)
        u = _trainer(torch, encoding, neurons, layers)
        for tr in (e, u):
            tr.gradients(*_batch(torch))
            buf = getattr(tr, name)
            assert bool(torch.isfinite(buf.float()).all()) and float(tr.dparams.abs().max()) > 0
            buf[buf.numel() // 2 + 1] = bad
        was = _state(e)
        e.apply_gradients()
        u.apply_gradients()
        torch.cuda.synchronize()
        assert _same(torch, was, _state(e)) == [], name
        assert all(not bool((g != 0).any()) for g in _grads(e)), name
        assert int(e.skipped_steps.item()) == 1 and e.step_count == 1
        assert not _finite(torch, _state(u)), f"{name}: the injected value did not poison the unguarded twin"
        twins.append(e)
    # a clean step behind the skipped one: finite, and the same bits whichever way the step was skipped
    G.step(*_batch(torch, 1))
    for e in twins:
        e.step(*_batch(torch, 1))
    torch.cuda.synchronize()
    ref = _state(G.tr["eager"])
    assert _finite(torch, ref) and _same(torch, before["eager"], ref) != []
    for p in ("captured", "entry"):
        assert _same(torch, ref, _state(G.tr[p])) == [], p
    for e in twins:
        assert _same(torch, ref, _state(e)) == []
    for tr in list(G.tr.values()) + twins:
        assert int(tr.skipped_steps.item()) == 1 and tr.step_count == 2


# ---- 8. resume and long runs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_resumed_run_continues_the_schedule(gpu, tmp_path, encoding, neurons, layers):
    torch = gpu
    kw = dict(lr_schedule=SCHED, weight_decay=0.01, skip_nonfinite=True)
    straight, half = (_trainer(torch, encoding, neurons, layers, **kw) for _ in range(2))
    for i in range(6):
        straight.step(*_batch(torch, i % 3))
    for i in range(4):
        half.step(*_batch(torch, i % 3))
    half._opt_guard[1] = 3                                      # as if three steps had been skipped
    path = str(tmp_path / "ck.rtxn")
    half.save_checkpoint(path)
    resumed = _trainer(torch, encoding, neurons, layers, **kw)
    header = resumed.load_checkpoint(path)
    assert header["skipped_steps"] == 3 and int(resumed.skipped_steps.item()) == 3 and resumed.step_count == 4
    assert resumed.current_lr() == half.current_lr() and ulps(resumed.current_lr(), np.float32(1e-2) * np.float32(factor64(5, **SCHED))) <= 1
    for i in range(4, 6):
        resumed.step(*_batch(torch, i % 3))
    torch.cuda.synchronize()
    assert _same(torch, _state(straight), _state(resumed)) == []
    plain = _trainer(torch, encoding, neurons, layers)          # a trainer without options reads the same file
    assert plain.load_checkpoint(path)["skipped_steps"] == 3 and plain.skipped_steps is None


def test_schedule_runs_past_the_captured_steps_rate_table(gpu):
    """step 70 001 is beyond the 2^16 entries the captured step without options looks its rate up in: with options the rate kernel
    evaluates schedule and bias correction from the counter itself, and the captured step uses the eager step's rate"""
    torch = gpu
    sched = dict(kind="exponential", decay_steps=100_000, ratio=0.1)
    P = _Paths(torch, "hash", 64, 4, which=("eager", "captured"), lr_schedule=sched)
    assert P.tr["captured"]._LR_TABLE < 70_000
    for tr in P.tr.values():
        tr.step_count = 70_000
    want = P.tr["eager"].current_lr()
    assert ulps(want, np.float32(1e-2) * np.float32(factor64(70_001, **sched))) <= 1 and want < 0.25e-2
    P.step(*_batch(torch))
    a, b = P.tr["eager"], P.tr["captured"]
    assert _same(torch, _state(a), _state(b)) == []
    for tr in (a, b):
        used = np.float32(1e-2) * np.float32(tr._opt_factor.item())
        print(f"rate used at step 70001: {float(used)!r}, current_lr() before the step {want!r}")
        assert ulps(used, want) <= 1              # device against host restatement: the rate kernel's 1 ulp
        assert tr.step_count == 70_001
