"""Early termination of the frame entry (RenderPipeline(min_transmittance=...), rtxn_render_set_termination): whole frames
against a float64 restatement of the round rule and of the compositors, fed with the PLAIN frame's own slot buffers.

The rule (include/rtxn.h): round k < N - 1 takes the next s0 * 2^k segments of every living ray, round N - 1 the rest; after
a round a ray stays alive iff it has segments left and T <= t_stop = -logf(eps), T being its optical depth after the last
shaded sample.  The outputs are the compositor's over the shaded prefix of each ray.

Inputs (weights seed, pose, step_scale, eps per schedule) were chosen on the CPU chain -- oracle.trace_packed + oracle.sample
+ oracle.mlp_forward (frequency models) resp. oracle.encode_hg + oracle.mlpe_forward (hash model), then _optical_depths and
_rule below -- so that at least a quarter of the hitting rays stop early, at least a quarter do not, and the rays whose
boundary T lies within 1e-4 (relative) of t_stop stay under 1 %.  Shares on that chain, as (stopped early, excluded) of the
hitting rays, for the schedules (1, 8) / (4, 5) / (2, 2):
  freq-8x128-compat (R 32, 828 hitting rays): (0.470, 0.0012) / (0.488, 0.0000) / (0.664, 0.0012)
  freq-2x64-compat  (R 64, 810 hitting rays): (0.485, 0.0012) / (0.505, 0.0000) / (0.509, 0.0000)
  hash-nerf         (R 32, 828 hitting rays): (0.557, 0.0000) / (0.506, 0.0000) / (0.507, 0.0000)
The Xavier-initialised 8 x 128 model's density is all but constant (sigma = 0.52 +- 0.01), so every ray reaches t_stop after the
same number of segments and no eps splits the (2, 2) schedule; its weights are therefore scaled by GAIN_8X128 = 1.5, which
spreads sigma over 0.75 .. 1.  The thresholds are small where a schedule's first boundaries lie deep in an opaque sphere: that
is what it takes for a quarter of the rays to be shaded to their end.
test_the_rule asserts the same three conditions on the GPU frame."""
import numpy as np
import pytest

from rtx_nerf_amd import scenes

pytestmark = pytest.mark.gpu
K32 = 32
BAR = 1e-5            # the project's compositor bar (tests/test_gpu_render_aux.py): absolute, pixels and opacity; depth x t_max
SCHEDULES = [(1, 8), (4, 5), (2, 2)]


# ------------------------------------------------------------------------------------------ float64 restatement
def _restate(rad, nh, idx, K, mode, t_hit, dist):
    """The compositors over the first nh[r] segments of each ray (tests/test_gpu_render_aux.py's restatement): rad
    float64[N, 4]; t_hit per sample (COMPAT: t_vals; NERF: step lengths); dist per sample.  pixels, opacity, depth."""
    B = len(nh)
    pix, acc, dep = np.zeros((B, 3)), np.zeros(B), np.zeros(B)
    for r in range(B):
        a, n = int(idx[r]) * K, int(nh[r]) * K
        if n == 0:
            continue
        c, t = rad[a:a + n], t_hit[a:a + n]
        if mode == 0:   # COMPAT: delta across the whole ray (t_{-1} = 0, not reset per segment), inclusive optical depth
            delta = np.abs(t - np.concatenate([[0.0], t[:-1]]))
            x = delta * c[:, 3]
            w = np.exp(-np.cumsum(x)) * (1 - np.exp(-x))
        else:
            x = t * c[:, 3]
            w = np.exp(-(np.cumsum(x) - x)) * (1 - np.exp(-x))
        pix[r] = (w[:, None] * c[:, :3]).sum(0)
        acc[r] = w.sum()
        dep[r] = (w * dist[a:a + n]).sum()
    return pix, acc, dep


def _optical_depths(rad, nh, idx, K, mode, t_hit):
    """Per ray: float64[nh[r]], the optical depth T after the last sample of each of its segments."""
    out = []
    for r in range(len(nh)):
        a, n = int(idx[r]) * K, int(nh[r]) * K
        c, t = rad[a:a + n], t_hit[a:a + n]
        if mode == 0:
            x = np.abs(t - np.concatenate([[0.0], t[:-1]])) * c[:, 3] if n else np.zeros(0)
        else:
            x = t * c[:, 3]
        out.append(np.cumsum(x)[K - 1::K])
    return out


def _rule(T, nh, s0, N, t_stop, margin=1e-4):
    """Segments each ray shades under the round rule, and the rays whose decision at some boundary lies within `margin`
    (relative) of t_stop: fp32 against float64 accumulation order may decide those either way."""
    shaded = np.zeros(len(nh), np.int64)
    unsure = np.zeros(len(nh), bool)
    for r in range(len(nh)):
        ns, done = int(nh[r]), 0
        if ns == 0:
            continue
        for k in range(N):
            done += min(s0 * 2 ** k, ns - done) if k < N - 1 else ns - done
            if done >= ns:
                break
            t = T[r][done - 1]
            if abs(t - t_stop) <= margin * t_stop:
                unsure[r] = True
                break
            if not t <= t_stop:
                break
        shaded[r] = done
    return shaded, unsure


# ------------------------------------------------------------------------------------------ frames
W, H = 96, 64
POSES = [scenes.pose_spherical(30.0, -30.0, origin_scale=10.0), scenes.pose_spherical(75.0, -20.0, origin_scale=10.0),
         scenes.pose_spherical(150.0, -45.0, origin_scale=10.0)]
# name: (grid_res, eps per schedule)
SETUPS = {
    "freq-8x128-compat": (32, {(1, 8): 3.162e-12, (4, 5): 5.623e-10, (2, 2): 0.065}),
    "freq-2x64-compat": (64, {(1, 8): 3e-12, (4, 5): 3e-11, (2, 2): 0.27}),
    "hash-nerf": (32, {(1, 8): 2e-5, (4, 5): 1e-4, (2, 2): 0.22}),
}
HASH_STEP_SCALE = 40.0
GAIN_8X128 = 1.5


def _occupancy(torch, R):
    return torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.7)).view(np.int32).copy()).cuda()


def _pipeline(torch, setup, **kw):
    from rtx_nerf_amd import api, render
    R = SETUPS[setup][0]
    f = scenes.lego_focal_length(True)
    kw.setdefault("max_segments", W * H * (40 if R == 32 else 80))
    kw.setdefault("aux", True)
    occ = _occupancy(torch, R)
    if setup.startswith("freq"):
        width, layers = (128, 8) if "8x128" in setup else (64, 2)
        net = api.Network(n_neurons=width, n_hidden_layers=layers)
        params = scenes.xavier_params_fp16(width, layers, 112, seed=1337)
        if width == 128:
            params = (params.astype(np.float32) * np.float32(GAIN_8X128)).astype(np.float16)
        net.set_params(torch.from_numpy(params).cuda())
        return render.RenderPipeline(net, R, W, H, f, occupancy=occ, **kw)
    hg = api.HashGrid(8, 2, 14, 8, 1.6, n_dir_freqs=4)
    E = hg.encoded_width()
    net = api.Network(n_neurons=64, n_hidden_layers=3, n_encoded_features=E)
    net.set_params(torch.from_numpy(scenes.xavier_params_fp16(64, 3, E, seed=5)).cuda())
    table = torch.from_numpy(np.random.default_rng(5).uniform(-0.5, 0.5, hg.n_params()).astype(np.float16)).cuda()
    p = render.RenderPipeline(net, R, W, H, f, occupancy=occ, vr_mode=api.VR_NERF, step_scale=HASH_STEP_SCALE, hashgrid=hg,
                              table=table, **kw)
    p._keep = (hg, net, table)
    return p


class _Plain:
    """The plain frame of `pipe` at `look_at` (termination off): its outputs and everything the restatement needs, on the host."""

    def __init__(self, torch, pipe, look_at, background=None, ray_begin=0):
        pipe.set_pose(look_at)
        n = pipe.max_rays
        self.out = tuple(t.clone() for t in pipe.render_ex(ray_begin=ray_begin, background=background))
        torch.cuda.synchronize()
        self.pix, self.dep, self.acc = (t.cpu().numpy() for t in self.out)
        K = K32
        self.nh_all = pipe.num_hits[:n].cpu().numpy()
        self.nh = pipe.num_hits_c[:n].cpu().numpy()
        self.idx = pipe.indices[:n].cpu().numpy()
        self.mode = pipe.vr_mode
        top = int((self.idx + self.nh)[self.nh > 0].max())
        start = pipe.start[:top].cpu().numpy().astype(np.float64)
        end = pipe.end[:top].cpu().numpy().astype(np.float64)
        self.rad = pipe.radiance[:top * K].float().cpu().numpy().astype(np.float64)
        if self.mode == 0:
            self.t_hit = (np.tile(np.arange(K), top) + 1) / K
        else:
            self.t_hit = np.repeat(pipe.seg_step[:top].cpu().numpy().astype(np.float64), K)
        la = np.asarray(look_at, np.float32).reshape(16)
        o = np.array([la[3] / np.float32(10), la[7] / np.float32(10), la[11] / np.float32(10)], np.float64)
        u = np.tile((np.arange(K) + (0.5 if pipe.sample_type == 3 else 0.0)) / K, top)
        p = np.repeat(start, K, axis=0) + u[:, None] * (np.repeat(end, K, axis=0) - np.repeat(start, K, axis=0))
        self.dist = np.linalg.norm(p - o[None, :], axis=1)
        self.t_max = float(np.linalg.norm(end - o[None, :], axis=1).max())
        self.T = _optical_depths(self.rad, self.nh, self.idx, K, self.mode, self.t_hit)

    def rule(self, eps, s0, N):
        return _rule(self.T, self.nh, s0, N, float(-np.log(np.float32(eps))))

    def truncated(self, shaded, background=None):
        pix, acc, dep = _restate(self.rad, shaded, self.idx, K32, self.mode, self.t_hit, self.dist)
        if background is not None:
            pix = pix + (1 - acc)[:, None] * np.asarray(background, np.float64)[None, :]
        return pix, acc, dep


def _terminated(torch, pipe, background=None, **kw):
    out = tuple(t.clone() for t in pipe.render_ex(background=background, **kw))
    torch.cuda.synchronize()
    return out, pipe.shaded_per_ray().cpu().numpy()


def _check_rule(plain, shaded, eps, s0, N, shares=True):
    want, unsure = plain.rule(eps, s0, N)
    hitting = plain.nh > 0
    n_hit = int(hitting.sum())
    early = hitting & (want < plain.nh) & ~unsure
    print(f"rule: eps {eps} schedule ({s0}, {N}): hitting {n_hit}, stopped early {early.sum() / n_hit:.3f}, "
          f"unsure {unsure.sum() / n_hit:.4f}, shaded share {want.sum() / plain.nh.sum():.3f}")
    assert unsure.sum() <= 0.01 * n_hit, "too many rays decide within 1e-4 of t_stop: the inputs do not test the rule"
    if shares:
        assert early.sum() >= 0.25 * n_hit and (hitting & (want == plain.nh) & ~unsure).sum() >= 0.25 * n_hit
    bad = np.flatnonzero((shaded != want) & ~unsure)
    assert bad.size == 0, f"{bad.size} rays shade another count than the rule, first {bad[:5]}: {shaded[bad[:5]]} vs {want[bad[:5]]}"
    assert (shaded[unsure] <= plain.nh[unsure]).all() and (shaded[~hitting] == 0).all()


def _check_parity(plain, out, shaded, background=None):
    pix, dep, acc = (t.cpu().numpy() for t in out)
    want_pix, want_acc, want_dep = plain.truncated(shaded, background)
    e = (np.abs(pix - want_pix).max(), np.abs(acc - want_acc).max(), np.abs(dep - want_dep).max() / plain.t_max)
    print(f"truncated parity: max |pixel| {e[0]:.2e}, |opacity| {e[1]:.2e}, |depth| / t_max {e[2]:.2e}")
    np.testing.assert_allclose(pix, want_pix, rtol=0, atol=BAR)
    np.testing.assert_allclose(acc, want_acc, rtol=0, atol=BAR)
    np.testing.assert_allclose(dep, want_dep, rtol=0, atol=BAR * plain.t_max)


# ------------------------------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("setup", list(SETUPS))
def test_off_is_off(gpu, setup):
    torch = gpu
    never = _pipeline(torch, setup)
    base = _Plain(torch, never, POSES[0])
    never.set_pose(POSES[0])
    base_pix = never.render().clone()
    pipe = _pipeline(torch, setup, min_transmittance=SETUPS[setup][1][(4, 5)])
    pipe.set_pose(POSES[0])
    # one round -- and, where no ray's optical depth comes near -log of the smallest eps a float holds (the hash frame: T < 30
    # against 85; the opaque frequency spheres reach 70 and 84), an eps that small: everything is shaded, and the outputs are
    # the plain frame's to the bar
    tiny = 1e-37
    cases = [(0.5, 4, 1), (tiny, 1, 1)]
    if setup == "hash-nerf":
        assert max(t.max() for t in base.T if t.size) < 0.5 * -np.log(np.float32(tiny))
        cases += [(tiny, 4, 5), (tiny, 1, 8)]
    for eps, s0, N in cases:
        pipe.set_termination(eps, s0, N)
        out, shaded = _terminated(torch, pipe)
        np.testing.assert_array_equal(shaded, base.nh)
        for got, want, bar in zip(out, base.out, (BAR, BAR * base.t_max, BAR)):
            np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=bar)
    # set, then cleared with NULL: the parent path bit for bit
    pipe.set_termination(None)
    out = tuple(t.clone() for t in pipe.render_ex())
    pix = pipe.render().clone()
    torch.cuda.synchronize()
    for got, want in zip(out, base.out):
        assert torch.equal(got, want)
    assert torch.equal(pix, base_pix)
    assert never.termination_stats()["frames"] == 0


# ------------------------------------------------------------------------------------------ 2. the rule
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("setup", list(SETUPS))
def test_the_rule(gpu, setup, schedule):
    torch = gpu
    s0, N = schedule
    eps = SETUPS[setup][1][schedule]
    pipe = _pipeline(torch, setup)
    plain = _Plain(torch, pipe, POSES[0])
    pipe.set_termination(eps, s0, N)
    _, shaded = _terminated(torch, pipe)
    _check_rule(plain, shaded, eps, s0, N)


# ------------------------------------------------------------------------------------------ 3. truncated parity
@pytest.mark.parametrize("background", [None, (1.0, 0.5, 0.25)])
@pytest.mark.parametrize("setup", list(SETUPS))
def test_truncated_parity(gpu, setup, background):
    torch = gpu
    eps = SETUPS[setup][1][(4, 5)]
    pipe = _pipeline(torch, setup)
    plain = _Plain(torch, pipe, POSES[0])
    pipe.set_termination(eps, 4, 5)
    out, shaded = _terminated(torch, pipe, background)
    assert (shaded < plain.nh).any()
    _check_parity(plain, out, shaded, background)
    # only the pixels requested: rtxn_render_frame is rtxn_render_frame_ex
    only, none_d, none_a = pipe.render_ex(depth=False, opacity=False)
    only = only.clone()
    pix = pipe.render().clone()
    torch.cuda.synchronize()
    assert none_d is None and none_a is None and torch.equal(only, pix)
    if background is None:
        assert torch.equal(pix, out[0])


# ------------------------------------------------------------------------------------------ 4. the bound
@pytest.mark.parametrize("setup", list(SETUPS))
def test_the_bound(gpu, setup):
    torch = gpu
    pipe = _pipeline(torch, setup)
    bg = (0.25, 1.0, 0.0)
    plain = _Plain(torch, pipe, POSES[0], background=bg)
    for schedule in SCHEDULES:
        eps = SETUPS[setup][1][schedule]
        pipe.set_termination(eps, *schedule)
        out, shaded = _terminated(torch, pipe, bg)
        pix, dep, acc = (t.cpu().numpy().astype(np.float64) for t in out)
        d_pix, d_acc, d_dep = np.abs(pix - plain.pix), plain.acc - acc, np.abs(dep - plain.dep)
        print(f"bound: eps {eps} {schedule}: max |pixel| {d_pix.max():.3e}, opacity {d_acc.min():.3e} .. {d_acc.max():.3e}, "
              f"|depth| / t_max {d_dep.max() / plain.t_max:.3e}")
        assert (d_pix <= eps + 2 * BAR).all()
        assert (0 <= d_acc + 2 * BAR).all() and (d_acc <= eps + 2 * BAR).all()
        assert (d_dep <= eps * plain.t_max + 2 * BAR * plain.t_max).all()
        assert (shaded < plain.nh).any() and d_acc.max() > 0


# ------------------------------------------------------------------------------------------ 5. stats, 6. capture
@pytest.mark.parametrize("setup", ["freq-2x64-compat", "hash-nerf"])
def test_stats_and_capture(gpu, setup):
    torch = gpu
    eps = SETUPS[setup][1][(4, 5)]
    pipe = _pipeline(torch, setup)
    plain = _Plain(torch, pipe, POSES[0])
    plain_total = int(pipe.total.item())
    assert plain_total == int(plain.nh.sum())
    pipe.set_termination(eps, 4, 5)
    assert pipe.termination_stats() == dict(frames=0, last_shaded_segments=0, last_total_segments=0, shaded_segments=0, total_segments=0)
    bg = (0.2, 0.3, 0.4)
    eager, shaded = _terminated(torch, pipe, bg)
    st = pipe.termination_stats()
    one = int(shaded.sum())
    assert st == dict(frames=1, last_shaded_segments=one, last_total_segments=plain_total, shaded_segments=one, total_segments=plain_total)
    assert 0 < one < plain_total
    g, pix, dep, acc = pipe.capture_ex(background=bg)
    base = pipe.termination_stats()
    assert base["frames"] == 1, "capturing a frame executes nothing"
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    for a, b in zip((pix, dep, acc), eager):
        assert torch.equal(a, b), "a replayed frame must be the eager frame bit for bit"
    st = pipe.termination_stats()
    assert st["frames"] == 4 and st["shaded_segments"] == 4 * one and st["total_segments"] == 4 * plain_total
    assert st["last_shaded_segments"] == one and st["last_total_segments"] == plain_total
    # a new pose written into the captured pose buffer
    for la in POSES[1:3]:
        pipe.set_pose(la)
        g.replay()
        got = (pix.clone(), dep.clone(), acc.clone())
        per_ray = pipe.shaded_per_ray().clone()
        want = tuple(t.clone() for t in pipe.render_ex(background=bg))
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert torch.equal(per_ray, pipe.shaded_per_ray())
    assert not torch.equal(got[0], eager[0])
    assert not pipe.overflowed()
    # the plain capture entry follows the setting too
    g2, pix2 = pipe.capture()
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(pix2, pipe.render_ex(depth=False, opacity=False)[0])


# ------------------------------------------------------------------------------------------ 7. truncation by capacity
@pytest.mark.parametrize("setup", ["freq-2x64-compat", "hash-nerf"])
def test_truncation_by_capacity(gpu, setup):
    torch = gpu
    s0, N = 4, 5
    eps = SETUPS[setup][1][(s0, N)]
    full = _pipeline(torch, setup)
    full.set_pose(POSES[0])
    need = full.count_segments()
    cap = need // 2
    pipe = _pipeline(torch, setup, max_segments=cap, on_overflow="ignore")
    plain = _Plain(torch, pipe, POSES[0])
    assert (plain.nh < plain.nh_all).any() and int(plain.nh.sum()) == cap
    pipe.set_termination(eps, s0, N)
    out, shaded = _terminated(torch, pipe)
    assert (shaded <= plain.nh).all() and (shaded < plain.nh).any()
    _check_rule(plain, shaded, eps, s0, N, shares=False)
    _check_parity(plain, out, shaded)
    st = pipe._status(wait=True)
    assert st.overflow_frames >= 2 and st.max_segments_needed == need and pipe.overflowed()
    ts = pipe.termination_stats()
    assert ts["last_total_segments"] == cap and ts["last_shaded_segments"] == int(shaded.sum())


# ------------------------------------------------------------------------------------------ 8. sharding
def test_windowed_shard_equals_the_full_frame_rows(gpu):
    torch = gpu
    setup = "hash-nerf"
    eps = SETUPS[setup][1][(4, 5)]
    bg = (1.0, 1.0, 1.0)
    full = _pipeline(torch, setup, min_transmittance=eps)
    full.set_pose(POSES[1])
    fp, fd, fa = (t.clone() for t in full.render_ex(background=bg))
    f_shaded = full.shaded_per_ray().clone()
    n_local = W * H // 2
    shard = _pipeline(torch, setup, window=(W, 2 * W), max_rays=n_local, min_transmittance=eps)
    shard.set_pose(POSES[1])
    sp, sd, sa = shard.render_ex(ray_begin=W, ray_count=n_local, background=bg)      # the odd image rows
    torch.cuda.synchronize()
    rows = np.arange(n_local)
    gid = torch.from_numpy(W + (rows // W) * 2 * W + rows % W).cuda()
    assert torch.equal(shard.shaded_per_ray(), f_shaded[gid])
    for a, b in ((sp, fp[gid]), (sd, fd[gid]), (sa, fa[gid])):
        assert torch.equal(a, b)
    assert float(sa.max()) > 0.05 and (f_shaded[gid] < full.num_hits_c[gid]).any()


# ------------------------------------------------------------------------------------------ 9. unsupported paths
def test_unsupported_paths(gpu):
    torch = gpu
    from rtx_nerf_amd import _lib, api, render
    net = api.Network(n_neurons=64, n_hidden_layers=2)
    net.set_params(torch.from_numpy(scenes.xavier_params_fp16(64, 2, 112, seed=1337)).cuda())
    f = scenes.lego_focal_length(True)
    kw = dict(occupancy=_occupancy(torch, 32), max_segments=W * H * 40)
    with pytest.raises(_lib.RtxnError, match="RTXN_RENDER_FLOAT4"):
        render.RenderPipeline(net, 32, W, H, f, compact=False, min_transmittance=1e-2, **kw)
    float4 = render.RenderPipeline(net, 32, W, H, f, compact=False, **kw)
    import ctypes as C
    t = _lib.RenderTermination(1e-2, 4, 5)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    assert _lib.lib().rtxn_render_set_termination(float4._h, C.byref(t), C.c_void_p(ws.data_ptr()), ws.numel()) == 3
    assert b"RTXN_RENDER_FLOAT4" in _lib.lib().rtxn_last_error()
    pipe = render.RenderPipeline(net, 32, W, H, f, min_transmittance=1e-2, n_slots=2, **kw)
    pose = torch.from_numpy(POSES[0].reshape(16).astype(np.float32)).cuda()
    for call in (lambda: pipe.render_async(pose), lambda: pipe.render_async(POSES[0]), lambda: pipe.render_async_ex(pose, depth=False),
                 lambda: pipe.render_async_ex(POSES[0], depth=False)):
        with pytest.raises(_lib.RtxnError, match="early termination is set"):
            call()
    # too small a workspace is an argument error, and clearing the setting gives the pipelined entries back
    assert _lib.lib().rtxn_render_set_termination(pipe._h, C.byref(t), C.c_void_p(ws.data_ptr()), 256) == 1
    assert b"workspace holds" in _lib.lib().rtxn_last_error()
    pipe.set_termination(None)
    pipe.set_pose(POSES[0])
    want = pipe.render().clone()
    pix, _, comp = pipe.render_async(pose)
    pipe.finish()
    assert torch.equal(pix, want)
