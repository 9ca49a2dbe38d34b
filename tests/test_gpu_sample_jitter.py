"""RTXN_SAMPLING_JITTER_WORLD on the GPU: the positions against a numpy restatement of include/rtxn.h's definition,
the folded consumers against the standalone sampler, the lean fused path against the staged one, the hash scatter against the
oracle's on the jittered samples (and NOT on the midpoints), the three stepping paths against each other, and the two things that
must not change: a trainer without jitter, and rendering.

Grid 16, sphere occupancy, one 30 x 30 camera batch: the segment count is no multiple of 8 (the backward's block tile), the sample
count no multiple of the padded unit, rays have odd segment counts (the sampler emits two per step) and the live list is a strict
subset -- asserted in _batch_shape_is_awkward, so the shapes cannot silently stop exercising them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, B, SEED = 16, 900, 21
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
U32 = np.uint32


# ---- the definition, restated (include/rtxn.h, "sample jitter") -----------------------------------------------------
def fmix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> U32(16)
    h *= U32(0x85EBCA6B)
    h ^= h >> U32(13)
    h *= U32(0xC2B2AE35)
    h ^= h >> U32(16)
    return h


def jitter_u(seed, step, n_samples):
    """u of samples 0 .. n_samples-1 as float32 (24 hash bits: exact)"""
    with np.errstate(over="ignore"):
        h0 = fmix32((U32(seed) ^ U32(0x5BD1E995)) + U32(0x9E3779B9) * U32(step))
        bits = fmix32(h0 ^ np.arange(n_samples, dtype=np.uint32)) >> U32(8)
    return bits.astype(np.float32) * np.float32(2.0 ** -24)


def jitter_positions(start, end, u):
    """(positions in float64: start + (i + u)/32 (end - start) without any fp32 rounding, t as the kernels form it in fp32)"""
    i = np.arange(u.size) % 32
    t32 = (i.astype(np.float32) + u) * np.float32(1.0 / 32)              # one fp32 rounding in the sum; the product is exact
    t64 = (i.astype(np.float64) + u.astype(np.float64)) / 32.0
    s0, s1 = np.repeat(start.astype(np.float64), 32, axis=0), np.repeat(end.astype(np.float64), 32, axis=0)
    return s0 + t64[:, None] * (s1 - s0), t32, s1


def _occ(torch):
    from rtx_nerf_amd import scenes
    return torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()


def _trainer(torch, encoding, neurons, layers, n_dir_freqs=4, **kw):
    from rtx_nerf_amd.train import Trainer
    kw.setdefault("sample_jitter", True)
    return Trainer(R, _occ(torch), encoding=encoding, n_neurons=neurons, n_hidden_layers=layers,
                   hashgrid=HGD if encoding == "hash" else None, n_dir_freqs=n_dir_freqs, batch_rays=B, max_segments=B * 30, lr=1e-2,
                   loss_scale=128.0, density_scale=120.0, mode="nerf", seed=3, jitter_seed=SEED, **kw)


_BATCHES = {}


def _batch(torch, i=0):
    """camera batch i and its targets, made once"""
    if i not in _BATCHES:
        from rtx_nerf_amd import scenes
        from rtx_nerf_amd.train import camera_rays
        o, d = camera_rays(scenes.pose_spherical(40.0 + 50.0 * i, -30.0 + 5.0 * i, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
        t = torch.from_numpy(np.random.default_rng(i).uniform(0, 1, (B, 3)).astype(np.float32)).cuda()
        _BATCHES[i] = (o, d, t)
    return _BATCHES[i]


def _randomise_table(torch, tr):
    g = torch.Generator().manual_seed(5)
    tr.table_master.copy_(((torch.rand(tr.hg.n_params(), generator=g) * 2 - 1) * 0.5).cuda())
    tr.table.copy_(tr.table_master.half())


def _rows(buf, E, S, capacity=None):
    """columns 0..S-1 of a feature-major tensor: the eager stages stride it by the batch's padded sample count, the one-call
    entry points by the capacity's"""
    from rtx_nerf_amd import api
    Sp = api.padded_samples(32 * capacity if capacity else S)
    return buf.reshape(-1)[:E * Sp].reshape(E, Sp)[:, :S]


def _live_columns(tr):
    segs = tr.live_ws[4:4 + int(tr.live_ws[0].item())].cpu().numpy().astype(np.int64)
    return (segs[:, None] * 32 + np.arange(32)[None, :]).reshape(-1)


def _batch_shape_is_awkward(torch, tr):
    from rtx_nerf_amd import api
    P = int(tr.total.item())
    assert P % 8 != 0 and (P * 32) % api.padded_samples(1) != 0
    assert int((tr.num_stored[:B] % 2 == 1).sum()) > 0
    if tr.live_segments:
        assert 0 < int(tr.live_ws[0].item()) < P
    return P


def _segments(tr, P):
    return tr.start[:P].cpu().numpy(), tr.end[:P].cpu().numpy()


# ---- 1. positions ------------------------------------------------------------------------------------------------------
def test_jittered_positions_match_the_definition(gpu):
    torch = gpu
    from rtx_nerf_amd import api
    tr = _trainer(torch, "hash", 64, 4)
    o, d, t = _batch(torch)
    tr.step_count = 5                                         # the step number is hashed: not 0
    S = tr.gradients(o, d, t)
    P = _batch_shape_is_awkward(torch, tr)
    assert S == 32 * P
    t_folded = tr.t_vals[:S].clone()
    tr.materialize_samples(B)
    got = tr.samples[:S].cpu().numpy()
    assert torch.equal(tr.t_vals[:S], t_folded)
    start, end = _segments(tr, P)
    want, t32, _ = jitter_positions(start, end, jitter_u(SEED, 5, S))
    err = np.abs(got[:, :3].astype(np.float64) - want).max()
    print(f"jittered positions: max |gpu - float64| = {err:.3e} (bound 2^-23 = {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23
    # every sample inside its stratum: in the kernels' own fp32 t, and as the positions the GPU wrote (slack: the position bound)
    i = np.arange(S) % 32
    assert np.array_equal(np.floor(t32 * np.float32(32)).astype(np.int64), i)
    seg = np.repeat((end - start).astype(np.float64), 32, axis=0)
    t_gpu = ((got[:, :3] - np.repeat(start, 32, axis=0).astype(np.float64)) * seg).sum(1) / (seg * seg).sum(1)
    slack = 32 * 2.0 ** -23 * np.sqrt(3.0) / np.sqrt((seg * seg).sum(1))
    assert (t_gpu * 32 >= i - slack).all() and (t_gpu * 32 < i + 1 + slack).all()
    assert np.abs(t_gpu * 32 - i - 0.5).mean() > 0.2          # spread over the stratum (uniform: 0.25), not the midpoints
    # t_vals: MIDPOINT_WORLD's, bit for bit
    tr.materialize_samples(B, jitter=None)
    assert torch.equal(tr.t_vals[:S], t_folded)
    mid = tr.samples[:S].clone()
    assert not torch.equal(mid[:, :3], torch.from_numpy(got[:, :3]).cuda()) and torch.equal(mid[:, 3:], torch.from_numpy(got[:, 3:]).cuda())
    # same (seed, step): same bits; another step: other positions; NULL step: step 0
    step = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    tr.materialize_samples(B, jitter=api.sample_jitter(SEED, step))
    assert np.array_equal(tr.samples[:S].cpu().numpy(), got)
    step.fill_(6)
    tr.materialize_samples(B, jitter=api.sample_jitter(SEED, step))
    other = tr.samples[:S].cpu().numpy()
    assert (other[:, :3] != got[:, :3]).any(axis=1).mean() > 0.99
    assert np.abs(other[:, :3].astype(np.float64) - jitter_positions(start, end, jitter_u(SEED, 6, S))[0]).max() <= 2.0 ** -23
    step.fill_(0)
    tr.materialize_samples(B, jitter=api.sample_jitter(SEED, step))
    zero = tr.samples[:S].clone()
    tr.materialize_samples(B, jitter=api.sample_jitter(SEED, None))
    assert torch.equal(tr.samples[:S], zero)
    assert np.abs(zero.cpu().numpy()[:, :3].astype(np.float64) - jitter_positions(start, end, jitter_u(SEED, 0, S))[0]).max() <= 2.0 ** -23


# ---- 2. folded = standalone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", ["hash", "freq"])
def test_folded_encoders_equal_the_standalone_sampler(gpu, oracle, monkeypatch, encoding):
    torch = gpu
    O = oracle
    o, d, t = _batch(torch)
    encs = []
    for fold in ("1", "0"):
        monkeypatch.setenv("RTXN_TRAIN_FOLD_SAMPLER", fold)
        tr = _trainer(torch, encoding, 64, 4)
        assert tr.fold_sampler == (fold == "1")
        if encoding == "hash":
            _randomise_table(torch, tr)
        tr.step_count = 2
        S = tr.gradients(o, d, t)
        P = int(tr.total.item())
        if fold == "1":
            _batch_shape_is_awkward(torch, tr)
            live = torch.from_numpy(_live_columns(tr)).cuda()
        encs.append((_rows(tr.encT, tr.E, S).clone(), tr.t_vals[:S].clone(), tr))
    (ea, ta, tra), (eb, tb, trb) = encs
    assert torch.equal(ta, tb)
    assert torch.equal(ea[:, live], eb[:, live]) and torch.equal(ea, eb)     # the live columns, and (forward: every column is written) all
    # both against the oracle's encoding of the numpy samples (view angles: the GPU's own atan2f)
    start, end = _segments(tra, P)
    pos, _, _ = jitter_positions(start, end, jitter_u(SEED, 2, S))
    trb.materialize_samples(B)
    samples = trb.samples[:S].cpu().numpy().copy()
    samples[:, :3] = pos.astype(np.float32)
    got = ea.t().contiguous().cpu().numpy().astype(np.float32)
    if encoding == "hash":
        want = O.encode_hg(O.hg_cfg(**HGD), 4, tra.table.cpu().numpy(), samples).astype(np.float32)
        # positions differ by one fp32 rounding (2^-24) times the finest level's scale and the table's slope: the bar of the chain
        # test's pixel comparison is far above it; here the encoding itself, at fp16 resolution of values <= 0.5
        err = np.abs(got - want).max()
        print(f"hash encoding vs oracle on the numpy samples: {err:.3e}")
        assert err < 2e-3
    else:
        want = O.encode_freq(O.mlp_cfg(n_neurons=64, n_hidden_layers=4), samples).astype(np.float32)
        err = np.abs(got - want).max()
        print(f"frequency encoding vs oracle on the numpy samples: {err:.3e}")
        assert err < 2e-3                                     # the bar test_gpu_training_loop uses for this stage


# ---- 3. lean fused path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [True, False])
def test_lean_fused_path_equals_the_staged_encoder_under_jitter(gpu, monkeypatch, deterministic):
    """8 x 128, 112 features: the forward's fused encoder and the weight gradient's own copy of the position (tpar) against the
    staged encoder, which reads what encode_freq_kernel wrote."""
    torch = gpu
    o, d, t = _batch(torch)
    runs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("RTXN_TRAIN_LEAN_FUSED", fused)
        tr = _trainer(torch, "freq", 128, 8, n_dir_freqs=12, deterministic=deterministic)
        assert tr.lean and tr.lean_fused == (fused == "1")
        tr.step_count = 3
        S = tr.gradients(o, d, t)
        _batch_shape_is_awkward(torch, tr)
        runs.append((tr.out[:S].clone(), tr.radiance[:S].clone(), tr.t_vals[:S].clone(), tr.dparams.clone()))
    a, b = runs
    for k in range(3):
        assert torch.equal(a[k], b[k]), ("out", "radiance", "t_vals")[k]
    assert float(a[3].abs().max()) > 0
    if deterministic:
        assert torch.equal(a[3], b[3]), f"{int((a[3] != b[3]).sum())} of {a[3].numel()} weight gradients differ"
    else:
        # the same operands bit for bit: the order of the fp32 atomic adds is what is left (the bars of
        # test_lean_backward_recomputing_the_encoding_equals_the_one_reading_it)
        x, y = a[3].double().cpu().numpy(), b[3].double().cpu().numpy()
        assert np.linalg.norm(x - y) <= 2e-5 * np.linalg.norm(x) and np.abs(x - y).max() <= 1e-4 * np.abs(x).max()
    # and the jitter is really there: the same step at the midpoints gives another forward
    monkeypatch.delenv("RTXN_TRAIN_LEAN_FUSED")
    if deterministic:
        mid = _trainer(torch, "freq", 128, 8, n_dir_freqs=12, sample_jitter=False)
        S = mid.gradients(o, d, t)
        assert torch.equal(mid.t_vals[:S], a[2]) and not torch.equal(mid.out[:S], a[0])


# ---- 4. the backward sees the forward's samples ---------------------------------------------------------------------------------
@pytest.mark.parametrize("live", ["1", "0"])
def test_hash_scatter_differentiates_the_jittered_samples(gpu, oracle, monkeypatch, live):
    torch = gpu
    O = oracle
    monkeypatch.setenv("RTXN_TRAIN_LIVE_SEGMENTS", live)
    tr = _trainer(torch, "hash", 64, 4, deterministic=True)
    assert tr.live_segments == (live == "1")
    _randomise_table(torch, tr)
    o, d, t = _batch(torch)
    tr.step_count = 4
    S = tr.gradients(o, d, t)
    P = _batch_shape_is_awkward(torch, tr)
    denc = _rows(tr.dencT, tr.E, S).t().contiguous().cpu().numpy()
    if tr.live_segments:                                      # d(encoding) of the segments the backward skipped was never written
        dead = np.ones(P, bool)
        dead[tr.live_ws[4:4 + int(tr.live_ws[0].item())].cpu().numpy()] = False
        denc[np.repeat(dead, 32)] = 0
    start, end = _segments(tr, P)
    got = tr.table_grad().cpu().numpy()
    ocfg = O.hg_cfg(**HGD)

    def gap(u):
        samples = np.zeros((S, 5), np.float32)
        samples[:, :3] = jitter_positions(start, end, u)[0].astype(np.float32)
        dt = O.hg_backward(ocfg, samples, denc)
        return np.abs(got - dt).max() / max(1e-6, np.abs(dt).max()), np.linalg.norm(got - dt) / np.linalg.norm(dt)

    mx, nrm = gap(jitter_u(SEED, 4, S))
    mx_mid, nrm_mid = gap(np.full(S, 0.5, np.float32))
    print(f"table gradient vs oracle: jittered samples max {mx:.3e} norm {nrm:.3e}; midpoint samples max {mx_mid:.3e} norm {nrm_mid:.3e}")
    bound = 2e-3 if tr.hash_fp16 else 1e-3
    assert mx < (1e-2 if tr.hash_fp16 else 1e-3) and nrm < bound      # the chain test's bounds
    # A scatter that ignored the jitter would have used the midpoints.  A sample moves by up to half a stratum (|segment| / 64, about
    # 1e-3 in world units, 1e-2 of a cell of the finest level), its eight weights by about as much, and an entry sums ~100 such
    # samples whose gradients differ in sign: 3e-3 ... 3e-2 of the norm.  So the midpoints must miss the chain test's bound, and
    # sit an order of magnitude away from what the right samples give (measured: 1.2e-4 against 3.2e-3, 26 times).
    assert nrm_mid > bound and nrm_mid > 10 * nrm


# ---- 5. three paths, one sequence -------------------------------------------------------------------------------------------------
def _three_paths(torch, encoding, neurons, layers):
    """three steps through step(), step_captured() and step_entry() from equal state, deterministic mode; yields after each step"""
    a, b, c = (_trainer(torch, encoding, neurons, layers, deterministic=True) for _ in range(3))
    b.capture_step(B, launch_segments=B * 30)
    c.entry_args(B, launch_segments=B * 30)
    for i in range(3):
        o, d, t = _batch(torch, i)
        a.step(o, d, t)
        S = int(a.total.item()) * 32
        ra = a.radiance[:S].clone()
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        b.step_captured()
        rb = b.radiance[:S].clone()
        c.graph_rays_o.copy_(o); c.graph_rays_d.copy_(d); c.graph_targets.copy_(t)
        c.step_entry()
        torch.cuda.synchronize()
        for name, x in (("captured", b), ("one-call", c)):
            for k, (p, q) in enumerate(((a.params, x.params), (a.master, x.master))):
                print(f"step {i}: eager vs {name}, {'params' if k == 0 else 'master'}: {int((p != q).sum())} of {p.numel()} differ, "
                      f"rel {float((p.float() - q.float()).norm()) / float(p.float().norm()):.2e}")
        yield i, a, b, c, ra, rb, c.radiance[:S].clone()
    assert a.step_count == b.step_count == c.step_count == 3


@pytest.mark.parametrize("encoding,neurons,layers", [("hash", 64, 4), ("freq", 128, 2)])
def test_eager_and_captured_steps_draw_the_same_offsets(gpu, encoding, neurons, layers):
    """step() and step_captured(): the same forward and the same parameters, bit for bit, after each of three steps -- and a
    midpoint trainer ends elsewhere."""
    torch = gpu
    for i, a, b, c, ra, rb, rc in _three_paths(torch, encoding, neurons, layers):
        assert float(ra.abs().max()) > 0 and torch.equal(ra, rb), f"forward, step {i}"
        assert torch.equal(a.params, b.params) and torch.equal(a.master, b.master), f"eager vs captured, step {i}"
    m = _trainer(torch, encoding, neurons, layers, deterministic=True, sample_jitter=False)
    for i in range(3):
        m.step(*_batch(torch, i))
    assert not torch.equal(m.master, a.master)


@pytest.mark.parametrize("encoding,neurons,layers", [("hash", 64, 4), ("freq", 128, 2)])
def test_eager_and_one_call_steps_draw_the_same_offsets(gpu, encoding, neurons, layers):
    """step() and step_entry(): the same forward and the same parameters, bit for bit, after each of three steps (the one-call
    step forms Adam's bias-corrected rate on the device, from powers taken in double so that it is the host's value)."""
    torch = gpu
    for i, a, b, c, ra, rb, rc in _three_paths(torch, encoding, neurons, layers):
        assert float(ra.abs().max()) > 0 and torch.equal(ra, rc), f"forward, step {i}"
        assert torch.equal(a.params, c.params) and torch.equal(a.master, c.master), f"eager vs one-call, step {i}"


# ---- 6. off is off -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers,ndf", [("hash", 64, 4, 4), ("freq", 128, 8, 12)])
def test_without_jitter_the_step_is_the_old_entry_points(gpu, encoding, neurons, layers, ndf):
    """sample_jitter=False: one step's encT, out, dparams and table gradient through the Trainer equal, bit for bit, the same step
    through the entry points that existed before the jitter, called directly over the same segments and loss gradients
    (deterministic mode; the same launch geometry, since a weight gradient's in-block sums follow it)."""
    torch = gpu
    from rtx_nerf_amd import api
    a = _trainer(torch, encoding, neurons, layers, n_dir_freqs=ndf, deterministic=True, sample_jitter=False)
    assert a._jitter(None) is None and a._stype() == api.SAMPLING_MIDPOINT_WORLD and a.live_segments
    M = api.SAMPLING_MIDPOINT_WORLD
    o, d, t = _batch(torch)
    if encoding == "hash":
        _randomise_table(torch, a)
    S = a.gradients(o, d, t)
    P = _batch_shape_is_awkward(torch, a)
    out, rad, tv, dp = torch.zeros_like(a.out), torch.zeros_like(a.radiance), torch.zeros_like(a.t_vals), torch.zeros_like(a.dparams)
    if encoding == "hash":
        assert a.recompute
        enc, denc = torch.zeros_like(a.encT), torch.zeros_like(a.dencT)
        a.hg.encode_segments(a.table, a.start, a.end, a.seg_view, P, M, enc, tv, a.density_scale)
        assert torch.equal(_rows(enc, a.E, S), _rows(a.encT, a.E, S))
        a.net.train_forward_outputs(enc, S, out, rad)
        a.net.train_backward_recompute_live(enc, out, a.dout, S, a.live_ws, dp, denc)
        dt = torch.zeros_like(a.dtable)
        dth = torch.zeros_like(a.dtable_h) if a.hash_fp16 else None
        a.hg.backward_segments(a.start, a.end, P, M, denc, dt, dth, live_ws=a.live_ws)
        if a.hash_fp16:
            dt[a.hashed_lo:] = dth.float()
        assert float(dt.abs().max()) > 0 and torch.equal(dt, a.table_grad())
    else:
        assert a.lean and a.lean_fused
        ws = a.net.train_lean_workspace(a.max_segments * 32)
        a.net.train_forward_lean_segments(a.start, a.end, a.seg_view, P, M, ws, out, rad, t_vals=tv, t_scale=a.density_scale)
        a.net.train_backward_lean_segments(a.start, a.end, a.seg_view, P, M, out, a.dout, ws, dp, live_ws=a.live_ws)
    torch.cuda.synchronize()
    assert torch.equal(out[:S], a.out[:S]) and torch.equal(rad[:S], a.radiance[:S]) and torch.equal(tv[:S], a.t_vals[:S])
    assert float(dp.abs().max()) > 0 and torch.equal(dp, a.dparams)


# ---- 7. rendering ignores it ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,neurons,layers,ndf", [("hash", 64, 4, 4), ("freq", 128, 8, 12)])
def test_rendering_ignores_the_jitter(gpu, encoding, neurons, layers, ndf):
    torch = gpu
    o, d, _ = _batch(torch, 1)
    a = _trainer(torch, encoding, neurons, layers, n_dir_freqs=ndf)
    b = _trainer(torch, encoding, neurons, layers, n_dir_freqs=ndf, sample_jitter=False)
    a.step_count = b.step_count = 7
    pa = a.render_rays(o, d).clone()
    pb = b.render_rays(o, d).clone()
    assert float(pa.abs().max()) > 0 and torch.equal(pa, pb)
    assert torch.equal(a.render_rays(o, d, background=(1.0, 0.5, 0.25)), b.render_rays(o, d, background=(1.0, 0.5, 0.25)))
