"""The weight EMA on the GPU (include/rtxn.h, rtxn_weight_ema): the dense and the lazy Adam kernels beside the _opt
kernels they are siblings of (Adam's own state bit for bit), the read-out against the float64 recurrence fed the GPU's own
sequence of weights, the read-out's purity, the skip word, the three stepping paths against each other, rendering from the
average, checkpoints, and "off is off".

The bar of every read-out is 8 * 2^-24 * max|w| / (1 - d) per buffer: an fp32 EMA step commits at most three roundings of
magnitude <= max|w|, the recurrence sums them geometrically, and the factor 8 leaves room for the debias division and the exp2.
Observed maxima are printed beside it.

Trainer shapes are those of test_gpu_optimizer.py: grid 16, sphere occupancy, 30 x 30 camera batches; hash 64 x 4 and the
frequency 8 x 128 model."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, B = 16, 900
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
MODELS = [("hash", 64, 4), ("freq", 128, 8)]
LS = 128.0
F = np.float32


def bar(d, w):
    return 8.0 * 2.0 ** -24 * float(np.abs(w).max()) / (1.0 - float(F(d)))


def _views(torch, n, offset, *dtypes):
    """zeroed tensors of n elements that start `offset` elements into their allocation (offset 1: no 16-byte alignment)"""
    return [torch.zeros(n + 8, dtype=dt, device="cuda")[offset:offset + n] for dt in dtypes]


class _Adam:
    """master, fp16 copy, both moments, per-entry counts, gradient, and (ema) accumulator and stamps, all at one offset"""

    def __init__(self, torch, n, offset, half_grads, w0):
        f32, f16, i32 = torch.float32, torch.float16, torch.int32
        self.master, self.params, self.m, self.v, self.steps, self.acc, self.stamps, self.grads = _views(
            torch, n, offset, f32, f16, f32, f32, i32, f32, i32, f16 if half_grads else f32)
        self.master.copy_(w0)
        self.params.copy_(w0.half())

    def adam_state(self):
        return [self.master, self.params, self.m, self.v, self.steps]


def _ema_fixture(torch, api, d, skip_nonfinite=False, **opt_kw):
    factor = torch.zeros(1, device="cuda")
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    opt = api.optimizer_options(opt_kw.get("sched"), opt_kw.get("weight_decay", 0.0), skip_nonfinite, factor, guard)
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    ema = api.weight_ema(d, state)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    rate = torch.zeros(1, device="cuda")
    return opt, guard, ema, state, step, rate


def _readout64(s64, w, d, u):
    """the debiased read-out in float64; u = 0: the weights"""
    return w.astype(np.float64) if u == 0 else s64 / (1.0 - np.float64(F(d)) ** np.float64(u))


def _check_f16(got16, want64):
    want16 = want64.astype(np.float16)
    err = np.abs(got16.astype(np.float64) - want16.astype(np.float64))
    assert (err <= np.spacing(np.abs(want16)).astype(np.float64)).all(), "fp16 read-out more than one fp16 ulp from the float64 one"


# ---- 1. the dense kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("half_grads", [False, True])
def test_dense_ema_kernel_leaves_adam_alone_and_reads_out_the_float64_recurrence(gpu, half_grads, offset):
    """n = 4 * 64 * 3 + 3: the vector body and the scalar tail; offset 1: everything through the scalar path.  A schedule and a
    decay term are switched on so that the EMA line sits behind both."""
    torch = gpu
    from rtx_nerf_amd import api
    n, steps, d, lr = 4 * 64 * 3 + 3, 40, 0.9, 1e-2
    rng = np.random.default_rng(11 + offset + 2 * half_grads)
    w0 = torch.from_numpy((rng.normal(size=n) * 0.1).astype(F)).cuda()
    a, b = _Adam(torch, n, offset, half_grads, w0), _Adam(torch, n, offset, half_grads, w0)
    opt, guard, ema, state, step, rate = _ema_fixture(torch, api, d, sched=dict(kind="exponential", warmup_steps=2, decay_start=2, decay_steps=8,
                                                                                ratio=0.5), weight_decay=0.01)
    s64 = np.zeros(n)
    d64 = np.float64(F(d))
    out32, out16 = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.float16, device="cuda")
    api.ema_weights(a.master, a.acc, None, state, d, out_f32=out32)
    assert torch.equal(out32, a.master), "u = 0 must read out the weights themselves"
    for u in range(1, steps + 1):
        g = torch.from_numpy((rng.normal(size=n) * LS * 0.01).astype(F)).cuda()
        a.grads.copy_(g)
        b.grads.copy_(g)
        api.optimizer_rate_ema(opt, ema, step, rate, lr=lr)          # one rate kernel: both sides read the same rate and factor
        api.adam_step_ema(a.master, a.params, a.grads, a.m, a.v, rate, opt, ema, a.acc, lr=lr, loss_scale=LS, zero_grads=True)
        api.adam_step_opt(b.master, b.params, b.grads, b.m, b.v, rate, opt, lr=lr, loss_scale=LS, zero_grads=True)
        s64 = d64 * s64 + (1.0 - d64) * a.master.cpu().numpy().astype(np.float64)
    for x, y, nm in zip(a.adam_state()[:4], b.adam_state()[:4], ("master", "params", "m", "v")):
        assert torch.equal(x, y), f"the EMA disturbed Adam: {nm}"
    assert not bool((a.grads != 0).any()) and int(state[0]) == steps and int(step[0]) == steps
    corr, host = F(state[1:2].view(torch.float32).item()), F(api.ema_correction(d, steps))        # double powers, rounded once: an ulp
    assert abs(int(corr.view(np.int32)) - int(host.view(np.int32))) <= 1
    acc_before = a.acc.clone()
    api.ema_weights(a.master, a.acc, None, state, d, out_f32=out32, out_f16=out16)
    w = a.master.cpu().numpy()
    want = _readout64(s64, w, d, steps)
    err = np.abs(out32.cpu().numpy().astype(np.float64) - want).max()
    print(f"dense read-out (half_grads={half_grads}, offset={offset}): max error {err:.3e}, bar {bar(d, w):.3e}")
    assert err <= bar(d, w)
    _check_f16(out16.cpu().numpy(), want)
    assert torch.equal(acc_before, a.acc)
    assert float(np.abs(want - w).max()) > 100 * bar(d, w), "the average never left the weights: the case tests nothing"


# ---- 2. the lazy kernel --------------------------------------------------------------------------------------------------------
N_SPARSE, ALWAYS, ONCE = 4099, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 4096), 13


def _pattern(rng, steps):
    """mask[step][i]: 10 % at random, then by construction: two whole quads, half of a third and the first tail element are touched
    every step; the rest of that third quad, every fifth element from 19 on and a tail element never; element 13 at the first and
    the last step only"""
    mask = rng.random((steps, N_SPARSE)) < 0.10
    never = np.zeros(N_SPARSE, dtype=bool)
    never[[10, 11, 4097]] = True
    never[19::5] = True
    never[list(ALWAYS)] = False
    mask[:, list(ALWAYS)] = True
    mask[:, never] = False
    mask[:, ONCE] = False
    mask[0, ONCE] = mask[steps - 1, ONCE] = True
    return mask, never


def _lazy64(ws, mask, w0, d, shift, jump=None):
    """the lazy form itself in float64 over the GPU's weights ws[u - 1] = w_u, with every gap moved by `shift`; returns the read-out"""
    d64 = np.float64(F(d))
    s, e, w_old, u = np.zeros(N_SPARSE), np.zeros(N_SPARSE, dtype=np.int64), w0.astype(np.float64), 0
    for k in range(len(ws)):
        if jump is not None and k == jump[0]:
            u = jump[1]
        u += 1
        t = mask[k]
        gap = np.maximum(u - 1 - e[t] + shift, 0)
        s[t] = w_old[t] + d64 ** gap * (s[t] - w_old[t])
        w_old = ws[k].astype(np.float64)
        s[t] = d64 * s[t] + (1.0 - d64) * w_old[t]
        e[t] = u
    gap = np.maximum(u - e + shift, 0)
    return (w_old + d64 ** gap * (s - w_old)) / (1.0 - d64 ** np.float64(u))


@pytest.mark.parametrize("d,half_grads,offset,jump", [(0.9, False, 0, None), (0.99, True, 0, None), (0.9, True, 1, None), (0.99, False, 1, None),
                                                      (0.9, False, 0, (30, 200_000))])
def test_lazy_ema_kernel_leaves_adam_alone_and_reads_out_the_dense_float64_recurrence(gpu, d, half_grads, offset, jump):
    """jump = (k, U): `updates` is set to U behind step k, as a resumed run would find it: the next gaps go through the
    large-exponent range of the exp2 (in float64 the k-th weights then simply stood for U - k updates)."""
    torch = gpu
    from rtx_nerf_amd import api
    n, steps, lr = N_SPARSE, 60, 1e-2
    rng = np.random.default_rng(int(d * 1000) + offset + 2 * half_grads)
    mask, never = _pattern(rng, steps)
    w0np = (rng.uniform(-1, 1, n) * 0.1).astype(F)
    w0 = torch.from_numpy(w0np).cuda()
    a, b = _Adam(torch, n, offset, half_grads, w0), _Adam(torch, n, offset, half_grads, w0)
    opt, guard, ema, state, step, rate = _ema_fixture(torch, api, d, sched=dict(warmup_steps=3))
    d64 = np.float64(F(d))
    s64, u, ws = np.zeros(n), 0, []
    for k in range(steps):
        if jump is not None and k == jump[0]:
            w = ws[-1].astype(np.float64)
            s64 = w + d64 ** np.float64(jump[1] - u) * (s64 - w)          # the weights stood still for jump[1] - u updates
            u = jump[1]
            state[0] = u
        u += 1
        g = np.where(mask[k], np.sign(rng.normal(size=n)) * (0.5 + rng.random(n)) * LS * 0.05, 0.0).astype(F)
        g = torch.from_numpy(g).cuda()
        a.grads.copy_(g)
        b.grads.copy_(g)
        api.optimizer_rate_ema(opt, ema, step, rate, lr=lr)
        api.adam_step_sparse_ema(a.master, a.params, a.grads, a.m, a.v, a.steps, opt, ema, a.acc, a.stamps, lr=lr, eps=1e-15, loss_scale=LS,
                                 zero_grads=True, weight_decay=False)
        api.adam_step_sparse_opt(b.master, b.params, b.grads, b.m, b.v, b.steps, opt, lr=lr, eps=1e-15, loss_scale=LS, zero_grads=True,
                                 weight_decay=False)
        ws.append(a.master.cpu().numpy())
        s64 = d64 * s64 + (1.0 - d64) * ws[-1].astype(np.float64)
    for x, y, nm in zip(a.adam_state(), b.adam_state(), ("master", "params", "m", "v", "param_steps")):
        assert torch.equal(x, y), f"the EMA disturbed Adam: {nm}"
    assert int(state[0]) == u and not bool((a.grads != 0).any())
    stamps = a.stamps.cpu().numpy()
    assert (stamps[list(ALWAYS)] == u).all() and (stamps[never] == 0).all() and stamps[ONCE] == u and int(a.steps[ONCE]) == 2
    assert torch.equal(a.master[torch.from_numpy(never).cuda()], w0[torch.from_numpy(never).cuda()])
    # the read-out: against the DENSE float64 recurrence over every element; pure
    acc_before, stamps_before, state_before = a.acc.clone(), a.stamps.clone(), state.clone()
    out32, out16 = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.float16, device="cuda")
    api.ema_weights(a.master, a.acc, a.stamps, state, d, out_f32=out32, out_f16=out16)
    w = ws[-1]
    want = _readout64(s64, w, d, u)
    got = out32.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"lazy read-out (d={d}, half_grads={half_grads}, offset={offset}, jump={jump}): max error {err:.3e}, bar {bar(d, w):.3e}")
    assert err <= bar(d, w)
    _check_f16(out16.cpu().numpy(), want)
    assert torch.equal(acc_before, a.acc) and torch.equal(stamps_before, a.stamps) and torch.equal(state_before, state), "the read-out is not pure"
    # never touched: the weight itself, to 2 ulp
    ulp = np.abs(got[never].astype(np.float64) - w[never].astype(np.float64)) / np.spacing(np.abs(w[never])).astype(np.float64)
    print(f"  never-touched entries: {int(never.sum())}, worst {ulp.max():.2f} ulp from their weight")
    assert ulp.max() <= 2.0
    # the float64 lazy form is the dense recurrence -- and with every gap off by one it MISSES the bar: the bar can tell
    assert np.abs(_lazy64(ws, mask, w0np, d, 0, jump) - want).max() < 1e-9 * np.abs(w).max()
    if jump is None:
        off = min(np.abs(_lazy64(ws, mask, w0np, d, shift, jump) - want).max() for shift in (1, -1))
        print(f"  gaps off by one: max error {off:.3e}")
        assert off > bar(d, w), "the negative control passes the bar: the bar is too wide to see a wrong gap"


# ---- 3. the skip word -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half_grads", [False, True])
def test_a_skipped_step_keeps_every_bit_of_the_average_and_clears_the_gradient(gpu, half_grads):
    torch = gpu
    from rtx_nerf_amd import api
    n, d, lr = 1031, 0.9, 1e-2
    rng = np.random.default_rng(5)
    w0 = torch.from_numpy((rng.normal(size=n) * 0.1).astype(F)).cuda()
    dense, lazy = _Adam(torch, n, 0, half_grads, w0), _Adam(torch, n, 0, half_grads, w0)
    opt, guard, ema, state, step, rate = _ema_fixture(torch, api, d, skip_nonfinite=True)

    def one(poison):
        g = np.where(rng.random(n) < 0.3, rng.normal(size=n) * LS * 0.05, 0.0).astype(F)
        if poison:
            g[n // 2] = np.inf
        for x in (dense, lazy):
            x.grads.copy_(torch.from_numpy(g).cuda())
        api.check_gradients([dense.grads, lazy.grads], guard)
        api.optimizer_rate_ema(opt, ema, step, rate, lr=lr)
        api.adam_step_ema(dense.master, dense.params, dense.grads, dense.m, dense.v, rate, opt, ema, dense.acc, lr=lr, loss_scale=LS, zero_grads=True)
        api.adam_step_sparse_ema(lazy.master, lazy.params, lazy.grads, lazy.m, lazy.v, lazy.steps, opt, ema, lazy.acc, lazy.stamps, lr=lr,
                                 eps=1e-15, loss_scale=LS, zero_grads=True)

    for _ in range(3):
        one(False)
    before = [t.clone() for t in dense.adam_state() + lazy.adam_state() + [dense.acc, lazy.acc, lazy.stamps, state]]
    one(True)
    after = dense.adam_state() + lazy.adam_state() + [dense.acc, lazy.acc, lazy.stamps, state]
    assert all(torch.equal(x, y) for x, y in zip(before, after)), "the skipped step moved the state"
    assert int(state[0]) == 3 and int(step[0]) == 4 and int(guard[1]) == 1 and int(guard[2]) == 1
    assert not bool((dense.grads != 0).any()) and not bool((lazy.grads != 0).any()) and not bool(torch.isnan(lazy.grads.float()).any())
    one(False)
    assert int(state[0]) == 4 and int(guard[2]) == 0 and not torch.equal(before[-3], lazy.acc) and bool(torch.isfinite(lazy.acc).all())
    # a rate call that does not advance the step counter only re-evaluates the rates: it is no update of the average
    was = state.clone()
    api.optimizer_rate_ema(opt, ema, step, rate, lr=lr, advance=False)
    assert torch.equal(was, state) and int(step[0]) == 5


# ---- 4. the Trainer --------------------------------------------------------------------------------------------------------------
def _occ(torch):
    from rtx_nerf_amd import scenes
    return torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()


def _trainer(torch, encoding, neurons, layers, **kw):
    from rtx_nerf_amd.train import Trainer
    kw.setdefault("deterministic", True)
    hgd = kw.pop("hashgrid", HGD)
    return Trainer(R, _occ(torch), encoding=encoding, n_neurons=neurons, n_hidden_layers=layers, hashgrid=hgd if encoding == "hash" else None,
                   n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2, loss_scale=LS, density_scale=120.0, mode="nerf", seed=3, **kw)


_BATCHES = {}


def _batch(torch, i=0, poisoned=False):
    """camera batch i and its targets, made once and never written"""
    if i not in _BATCHES:
        from rtx_nerf_amd import scenes
        from rtx_nerf_amd.train import camera_rays
        o, d = camera_rays(scenes.pose_spherical(40.0 + 50.0 * i, -30.0 + 5.0 * i, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
        t = torch.from_numpy(np.random.default_rng(i).uniform(0, 1, (B, 3)).astype(F)).cuda()
        _BATCHES[i] = (o, d, t)
    o, d, t = _BATCHES[i]
    if poisoned:
        t = t.clone()
        t[:, 0] = float("inf")              # targets feed only the loss: arithmetic, never an index
    return o, d, t


def _state(tr):
    names = ["master", "params", "adam_m", "adam_v"] + (["table_master", "table", "table_m", "table_v", "table_steps"] if tr.encoding == "hash" else [])
    return {k: getattr(tr, k).clone() for k in names}


def _ema_state(tr):
    names = ["_ema_state", "ema_mlp"] + (["ema_table", "ema_stamps"] if tr.encoding == "hash" else [])
    return {k: getattr(tr, k).clone() for k in names}


def _same(torch, a, b):
    """names of the tensors that differ"""
    return [k for k in a if not torch.equal(a[k], b[k])]


_SEGMENTS = {}


def _segments(torch, i=0):
    """the number of segments camera batch i cuts out of the occupancy grid (a property of the rays alone), counted once"""
    if i not in _SEGMENTS:
        tr = _trainer(torch, "freq", 128, 2)
        o, d, _ = _batch(torch, i)
        tr.render_rays(o, d)
        _SEGMENTS[i] = int(tr.total.item())
    return _SEGMENTS[i]


def _lean(encoding, neurons, layers):
    """the 8 x 128 frequency model trains on the lean path, whose weight gradient sums in fp32 inside a block before the blocks
    meet in fixed point: the bits of a step follow the launch geometry (tests/test_gpu_sample_jitter.py pins it for that reason).
    The eager step sizes its launches by the batch's segment count, the captured and the one-call step by launch_segments -- at
    B * 30 the eager step's live weights differ from the other two's by 7.9e-9 in relative norm after one step and 4.6e-2 after
    twenty, with or without ema_decay, and did before the EMA existed (profiles/r15/three_paths_8x128.txt).  What the three-path
    tests are about is the average, so on this model they give all three paths ONE geometry: every step takes the rays of camera
    batch 0 (the targets still change from step to step) and the captured and one-call steps are sized for exactly that batch's
    segment count.  The other models keep three camera batches and B * 30."""
    return (encoding, neurons, layers) == ("freq", 128, 8)


def _step_batch(torch, encoding, neurons, layers, i, poisoned=False):
    """the batch of step i of a three-path run (see _lean)"""
    o, d, t = _batch(torch, i % 3, poisoned=poisoned)
    if _lean(encoding, neurons, layers):
        o, d, _ = _batch(torch, 0)
    return o, d, t


class _Paths:
    """one trainer behind each of the three stepping methods"""

    def __init__(self, torch, encoding, neurons, layers, which=("eager", "captured", "entry"), **kw):
        self.torch = torch
        self.tr = {p: _trainer(torch, encoding, neurons, layers, **kw) for p in which}
        launch = _segments(torch, 0) if _lean(encoding, neurons, layers) else B * 30
        if "captured" in self.tr:
            self.tr["captured"].capture_step(B, launch_segments=launch)
        if "entry" in self.tr:
            self.tr["entry"].entry_args(B, launch_segments=launch)

    def step(self, o, d, t):
        for p, tr in self.tr.items():
            _step(tr, p, o, d, t)
        self.torch.cuda.synchronize()


def _step(tr, path, o, d, t):
    if path == "eager":
        tr.step(o, d, t)
    else:
        tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
        tr.step_captured() if path == "captured" else tr.step_entry()


@pytest.mark.parametrize("encoding,neurons,layers", MODELS + [("freq", 128, 2)])
def test_three_paths_keep_one_average_and_leave_the_live_weights_alone(gpu, encoding, neurons, layers):
    """20 steps, ema_decay=0.9, skip_nonfinite=True: eager, captured and one-call steps end with bit-identical s, stamps and
    ema_updates, and the live weights are those of the same trainer without ema_decay.  The 8 x 128 model runs at one launch
    geometry on all three paths (_lean says why); 128 x 2 is a third model, where the paths agree at any geometry."""
    torch = gpu
    P = _Paths(torch, encoding, neurons, layers, ema_decay=0.9, skip_nonfinite=True)
    plain = _trainer(torch, encoding, neurons, layers, skip_nonfinite=True)
    for i in range(20):
        P.step(*_step_batch(torch, encoding, neurons, layers, i))
        plain.step(*_step_batch(torch, encoding, neurons, layers, i))
    a, c, e = P.tr["eager"], P.tr["captured"], P.tr["entry"]
    assert not any(tr.truncated_steps for tr in P.tr.values())
    assert all(int(tr.ema_updates.item()) == 20 and tr.step_count == 20 and int(tr.skipped_steps.item()) == 0 for tr in P.tr.values())
    assert _same(torch, _state(plain), _state(a)) == [], "the EMA moved the live weights"
    assert _same(torch, _ema_state(c), _ema_state(e)) == [] and _same(torch, _state(c), _state(e)) == [], "captured vs entry"
    mlp, table = a.ema_parameters()
    assert bool(torch.isfinite(mlp).all()) and not torch.equal(mlp, a.master) and (table is None) == (encoding != "hash")
    if table is not None:
        assert bool(torch.isfinite(table).all()) and not torch.equal(table, a.table_master)
        never = a.ema_stamps == 0
        assert bool(never.any()) and bool((a.ema_stamps == 20).any())
        assert float(((table - a.table_master)[never].abs() / a.table_master[never].abs().clamp_min(1e-30)).max()) < 4 * 2.0 ** -24
    for p in ("captured", "entry"):
        assert _same(torch, _ema_state(a), _ema_state(P.tr[p])) == [], f"eager vs {p}: the average"
        assert _same(torch, _state(a), _state(P.tr[p])) == [], f"eager vs {p}: the live weights"


@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_a_step_the_guard_skips_does_not_count_on_any_path(gpu, encoding, neurons, layers):
    """an Inf planted in a target at step 7: ema_updates == 19 on every path, the skipped step moved no bit of the average, and
    the three paths end with the same average"""
    torch = gpu
    P = _Paths(torch, encoding, neurons, layers, ema_decay=0.9, skip_nonfinite=True)
    for i in range(20):
        if i == 6:                                             # step 7
            before = {p: _ema_state(tr) for p, tr in P.tr.items()}
        P.step(*_step_batch(torch, encoding, neurons, layers, i, poisoned=(i == 6)))
        if i == 6:
            for p, tr in P.tr.items():
                assert _same(torch, before[p], _ema_state(tr)) == [], f"{p}: the skipped step moved the average"
                assert int(tr.ema_updates.item()) == 6 and int(tr.skipped_steps.item()) == 1, p
    for p, tr in P.tr.items():
        assert int(tr.ema_updates.item()) == 19 and tr.step_count == 20 and int(tr.skipped_steps.item()) == 1, p
        assert all(bool(torch.isfinite(v.float()).all()) for v in {**_state(tr), **_ema_state(tr)}.values())
    for p in ("captured", "entry"):
        assert _same(torch, _ema_state(P.tr["eager"]), _ema_state(P.tr[p])) == [], p


def test_the_three_stepping_methods_of_one_trainer_share_the_average(gpu):
    _mixed_against_eager(gpu)


def test_the_three_stepping_methods_share_the_average_on_a_one_feature_grid(gpu):
    """five levels of ONE feature: an odd level count, the fp32 scatter, and four table entries per quad of the lazy kernel"""
    mixed = _mixed_against_eager(gpu, hashgrid=dict(HGD, n_levels=5, n_features=1))
    assert mixed.hg.cfg.n_features == 1 and not mixed.hash_fp16
    assert bool((mixed.ema_stamps == 0).any()) and bool((mixed.ema_stamps == 6).any())


def _mixed_against_eager(gpu, **kw):
    torch = gpu
    mixed, eager = (_trainer(torch, "hash", 64, 4, ema_decay=0.9, skip_nonfinite=True, **kw) for _ in range(2))
    mixed.capture_step(B, launch_segments=B * 30)
    mixed.entry_args(B, launch_segments=B * 30)
    for i, p in enumerate(("eager", "captured", "entry", "captured", "eager", "entry")):
        _step(mixed, p, *_batch(torch, i % 3))
        eager.step(*_batch(torch, i % 3))
    torch.cuda.synchronize()
    assert int(mixed.ema_updates.item()) == 6
    assert _same(torch, _ema_state(eager), _ema_state(mixed)) == [] and _same(torch, _state(eager), _state(mixed)) == []
    return mixed


def test_dense_table_rule_keeps_the_table_average_densely(gpu, monkeypatch):
    """RTXN_TABLE_ADAM=dense: every table entry moves every step, so the table's average takes the dense kernel and needs no
    stamps; eager and captured (the one-call step has no dense rule) agree, and the read-out is the float64 recurrence."""
    torch = gpu
    monkeypatch.setenv("RTXN_TABLE_ADAM", "dense")
    P = _Paths(torch, "hash", 64, 4, which=("eager", "captured"), ema_decay=0.9, skip_nonfinite=True)
    plain = _trainer(torch, "hash", 64, 4, skip_nonfinite=True)
    a, c = P.tr["eager"], P.tr["captured"]
    assert not a.table_adam_sparse and a.ema_stamps is None and a.ema_table is not None
    d64, s64 = np.float64(F(0.9)), np.zeros(a.table_master.numel())
    for i in range(8):
        P.step(*_batch(torch, i % 3))
        plain.step(*_batch(torch, i % 3))
        s64 = d64 * s64 + (1.0 - d64) * a.table_master.cpu().numpy().astype(np.float64)
    names = ["_ema_state", "ema_mlp", "ema_table"]
    assert [k for k in names if not torch.equal(getattr(a, k), getattr(c, k))] == [] and _same(torch, _state(a), _state(c)) == []
    assert _same(torch, _state(plain), _state(a)) == [] and int(a.ema_updates.item()) == 8
    _, table = a.ema_parameters()
    w = a.table_master.cpu().numpy()
    err = np.abs(table.cpu().numpy().astype(np.float64) - _readout64(s64, w, 0.9, 8)).max()
    print(f"dense table read-out: max error {err:.3e}, bar {bar(0.9, w):.3e}")
    assert err <= bar(0.9, w) and not torch.equal(table, a.table_master)


# ---- 5. rendering ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_render_pipeline_draws_the_average_and_the_live_frame_stays(gpu, encoding, neurons, layers):
    torch = gpu
    from rtx_nerf_amd import api, render, scenes
    W = H = 32
    f, la = scenes.lego_focal_length(True), scenes.pose_spherical(30.0, -30.0, origin_scale=10.0)
    tr = _trainer(torch, encoding, neurons, layers, ema_decay=0.9)
    for i in range(10):
        tr.step(*_batch(torch, i % 3))
    tr.sync_inference_weights()
    with pytest.raises(RuntimeError, match="sync_ema"):
        tr.render_pipeline(W, H, f, max_segments=W * H * 40, weights="ema")
    live = tr.render_pipeline(W, H, f, max_segments=W * H * 40)
    live.set_pose(la)
    first = live.render().clone()
    training = {**_state(tr), **_ema_state(tr)}
    tr.sync_ema()
    pipe = tr.render_pipeline(W, H, f, max_segments=W * H * 40, weights="ema")
    pipe.set_pose(la)
    frame = pipe.render().clone()
    # a fresh model set to ema_parameters()
    mlp, table = tr.ema_parameters()
    c = tr.net.cfg
    net = api.Network(n_neurons=c.n_neurons, n_hidden_layers=c.n_hidden_layers, n_pos_freqs=c.n_pos_freqs, n_dir_freqs=c.n_dir_freqs,
                      n_pos_dims=c.n_pos_dims, n_dir_dims=c.n_dir_dims, n_output_dims=c.n_output_dims, output_activation=c.output_activation,
                      n_encoded_features=c.n_encoded_features)
    net.set_params(mlp.half())
    kw = dict(hashgrid=tr.hg, table=table.half()) if encoding == "hash" else {}
    fresh = render.RenderPipeline(net, R, W, H, f, occupancy=tr.occ, max_segments=W * H * 40, vr_mode=api.VR_NERF, step_scale=tr.density_scale, **kw)
    fresh.set_pose(la)
    want = fresh.render().clone()
    torch.cuda.synchronize()
    assert not pipe.overflowed() and bool(torch.isfinite(frame).all()) and float(frame.abs().max()) > 0
    assert torch.equal(frame, want), "the ema pipeline does not draw ema_parameters()"
    assert not torch.equal(frame, first), "the averaged frame is the live frame"
    assert torch.equal(live.render(), first), "sync_ema() moved the live frame"
    assert _same(torch, training, {**_state(tr), **_ema_state(tr)}) == [], "reading the average out changed the training state"


# ---- 6. checkpoints ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_resumed_run_continues_the_average(gpu, tmp_path, encoding, neurons, layers):
    torch = gpu
    kw = dict(ema_decay=0.9, skip_nonfinite=True)
    straight, half = (_trainer(torch, encoding, neurons, layers, **kw) for _ in range(2))
    for i in range(20):
        straight.step(*_batch(torch, i % 3))
    for i in range(10):
        half.step(*_batch(torch, i % 3))
    path = str(tmp_path / "ck.rtxn")
    half.save_checkpoint(path)
    resumed = _trainer(torch, encoding, neurons, layers, **kw)
    resumed.load_checkpoint(path)
    assert int(resumed.ema_updates.item()) == 10 and _same(torch, _ema_state(half), _ema_state(resumed)) == []
    for i in range(10, 20):
        resumed.step(*_batch(torch, i % 3))
    torch.cuda.synchronize()
    assert _same(torch, _state(straight), _state(resumed)) == [] and _same(torch, _ema_state(straight), _ema_state(resumed)) == []
    # both ways round: a trainer without the EMA reads the same file, and a file without the EMA starts the average at u = 0
    plain = _trainer(torch, encoding, neurons, layers, skip_nonfinite=True)
    plain.load_checkpoint(path)
    assert _same(torch, _state(half), _state(plain)) == [] and plain.ema_updates is None
    bare = str(tmp_path / "bare.rtxn")
    plain.save_checkpoint(bare)
    resumed.load_checkpoint(bare)
    assert int(resumed.ema_updates.item()) == 0 and all(not bool((v != 0).any()) for v in _ema_state(resumed).values())
    mlp, _ = resumed.ema_parameters()
    assert torch.equal(mlp, resumed.master)


def test_an_average_kept_another_way_is_not_continued(gpu, tmp_path, monkeypatch):
    """the header holds the decay and the form of the table's average; a file whose average was kept with another decay, or lazily
    where this trainer keeps it densely (or the other way round), starts the average over at u = 0 and says so -- a lazy
    accumulator read as a dense one would be stale wherever Adam did not touch it.  The weights load all the same."""
    torch = gpu
    lazy = _trainer(torch, "hash", 64, 4, ema_decay=0.9)
    for i in range(4):
        lazy.step(*_batch(torch, i % 3))
    path = str(tmp_path / "lazy.rtxn")
    lazy.save_checkpoint(path)
    same = _trainer(torch, "hash", 64, 4, ema_decay=0.9)
    assert same.load_checkpoint(path)["weight_ema"] == {"decay": float(F(0.9)), "table": "lazy"}
    assert int(same.ema_updates.item()) == 4 and _same(torch, _ema_state(lazy), _ema_state(same)) == []
    other = _trainer(torch, "hash", 64, 4, ema_decay=0.99)
    with pytest.warns(UserWarning, match="starts over"):
        other.load_checkpoint(path)
    assert int(other.ema_updates.item()) == 0 and all(not bool((v != 0).any()) for v in _ema_state(other).values())
    assert _same(torch, _state(lazy), _state(other)) == []
    monkeypatch.setenv("RTXN_TABLE_ADAM", "dense")
    dense = _trainer(torch, "hash", 64, 4, ema_decay=0.9)
    assert dense.ema_stamps is None
    with pytest.warns(UserWarning, match="starts over"):
        dense.load_checkpoint(path)
    assert int(dense.ema_updates.item()) == 0 and not bool((dense.ema_table != 0).any()) and not bool((dense.ema_mlp != 0).any())
    for i in range(2):
        dense.step(*_batch(torch, i))
    back = str(tmp_path / "dense.rtxn")
    dense.save_checkpoint(back)
    monkeypatch.delenv("RTXN_TABLE_ADAM")
    again = _trainer(torch, "hash", 64, 4, ema_decay=0.9)
    with pytest.warns(UserWarning, match="starts over"):
        again.load_checkpoint(back)
    assert int(again.ema_updates.item()) == 0 and all(not bool((v != 0).any()) for v in _ema_state(again).values())


# ---- 7. off is off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers", MODELS)
def test_without_ema_decay_nothing_is_allocated_and_every_path_is_unchanged(gpu, encoding, neurons, layers):
    """What this can show: ema_decay=None allocates nothing, keeps the options struct away and refuses the read-outs.  Its
    bit-for-bit half compares two trainers of THIS build, so it shows only that the argument itself changes nothing; that a
    trainer without ema_decay behaves as it did before the EMA existed is what the unchanged suites of the other features pin
    (their three-path and "off is off" tests run the same kernels through the same calls)."""
    torch = gpu
    base = _Paths(torch, encoding, neurons, layers)
    none = _Paths(torch, encoding, neurons, layers, ema_decay=None)
    for tr in none.tr.values():
        assert tr.ema_decay is None and tr.ema_updates is None and tr._ema is None and tr._ema_state is None
        assert tr.ema_mlp is None and tr.ema_table is None and tr.ema_stamps is None and tr._opt is None
        with pytest.raises(RuntimeError, match="ema_decay"):
            tr.ema_parameters()
        with pytest.raises(RuntimeError, match="ema_decay"):
            tr.sync_ema()
    for i in range(5):
        base.step(*_batch(torch, i % 3))
        none.step(*_batch(torch, i % 3))
    for p in ("eager", "captured", "entry"):
        assert _same(torch, _state(base.tr[p]), _state(none.tr[p])) == [], p
