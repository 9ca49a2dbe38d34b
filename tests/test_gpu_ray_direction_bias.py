"""Layer 0's view-direction product once per RAY (rtxn_mlp_ray_direction_bias, rtxn_mlp_forward_segments_rays*): a segment's
direction is its ray's, so the frame of a 64 / 128-wide frequency model forms the W values once per ray with a hit, on the
traversal stream, and the segment kernel starts layer 0 from the ray's row of that table instead of multiplying the
direction k-steps per segment.  The values are the same encoder's, the same MFMA's, in the same k order: everything below
is exact (torch.equal) against the seg_view entries, which keep the per-segment product.

Shapes: a 32^3 sphere, 48 x 40 rays (pose 30: 4,612 segments = 288 tiles and 4 segments, 239 rays with a hit, 11 of them with
exactly one segment, 195 whose segments straddle a 16-segment tile; pose 200: 4,419 segments), the persistent grid shrunk to
CUs - 64 blocks so that blocks take a second tile.  The preconditions are asserted, not assumed."""
import ctypes as C

import numpy as np
import pytest

from rtx_nerf_amd import scenes

R, W_IMG, H_IMG = 32, 48, 40
VARIANTS = [(128, 12), (64, 12), (128, 4), (64, 4)]      # (width, direction frequencies): the four fwd16 kernels
DEPTHS = [1, 2, 3, 8]
POISON = -7.0


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _params(W, depth, E, seed):
    return scenes.xavier_params_fp16(W, depth, E, seed=seed)


def _net(torch, api, W, df, depth, seed=3, reserved=64):
    net = api.Network(n_neurons=W, n_hidden_layers=depth, n_dir_freqs=df)
    net.set_params(_dev(torch, _params(W, depth, net.encoded_width(), seed)))
    net.set_reserved_cus(reserved)
    return net


def _pose(az):
    return scenes.pose_spherical(az, -30.0, origin_scale=10.0)


@pytest.fixture(scope="module")
def scene(gpu):
    torch = gpu
    words = scenes.pack_occupancy(scenes.sphere_density(R, 0.6))
    return dict(occ=torch.from_numpy(words.view(np.int32).copy()).cuda(), focal=scenes.lego_focal_length(True))


def _pipe(scene, net, **kw):
    from rtx_nerf_amd import render
    kw.setdefault("max_segments", 6000)
    return render.RenderPipeline(net, R, W_IMG, H_IMG, scene["focal"], occupancy=scene["occ"], **kw)


def _reshade_with_seg_view(torch, pipe, g):
    """The slot's segments through the PUBLIC seg_view entry (per-segment product), into a buffer of its own."""
    out = torch.full_like(g.radiance, POISON)
    if pipe.compact:
        pipe.net.forward_segments_compact(g.start, g.end, g.seg_view, g.total, pipe.max_segments, out)
        return out, None
    tv = torch.full_like(g.t_vals, POISON)
    pipe.net.forward_segments(g.start, g.end, g.seg_view, g.total, pipe.max_segments, out, tv)
    return out, tv


# ---------------------------------------------------------------------------------------------------- the kernels alone
@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("W,df", VARIANTS)
def test_ray_entries_equal_the_seg_view_entries(gpu, W, df, depth):
    """Synthetic segments whose rays are NOT in packed order (a permutation, several segments per ray, rays without any):
    both output forms equal the seg_view entries given seg_view[k] = view[seg_ray[k]]; nothing past *total_segments or
    max_segments is written; the rows of rays without a hit keep their poison."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(100 * W + 10 * df + depth)
    n_rays, total, max_segments, cap = 211, 5003, 4990, 5040       # 312 tiles: grid of CUs - 64 blocks, second tiles; odd live count
    net = _net(torch, api, W, df, depth, seed=11 + depth)
    assert net.ray_direction_bias_supported()
    view = np.stack([rng.uniform(0, 3.1416, n_rays), rng.uniform(-3.1416, 3.1416, n_rays)], axis=1).astype(np.float32)
    hit = rng.uniform(size=n_rays) < 0.7
    hit[[0, n_rays - 1]] = True
    seg_ray = rng.choice(np.flatnonzero(hit), cap).astype(np.int32)
    seg_ray[1] = seg_ray[0]                                         # a wave whose two segments share a ray
    sp = rng.uniform(-1, 1, (cap, 3)).astype(np.float32)
    ep = rng.uniform(-1, 1, (cap, 3)).astype(np.float32)
    num_hits = np.where(hit, 1, 0).astype(np.int32)
    table = torch.full((n_rays, W), POISON, device="cuda")
    net.ray_direction_bias(_dev(torch, view), _dev(torch, num_hits), table)
    assert bool((table[_dev(torch, ~hit)] == POISON).all()) and bool((table[_dev(torch, hit)] != POISON).any(dim=1).all())
    tot = torch.tensor([total], dtype=torch.int32, device="cuda")
    sp_d, ep_d, sr_d, sv_d = _dev(torch, sp), _dev(torch, ep), _dev(torch, seg_ray), _dev(torch, view[seg_ray])
    for dtype in (torch.float16, torch.float32):
        got = torch.full((cap * 32, 4), POISON, dtype=dtype, device="cuda")
        want = torch.full((cap * 32, 4), POISON, dtype=dtype, device="cuda")
        if dtype == torch.float16:
            net.forward_segments_rays(sp_d, ep_d, sr_d, table, tot, max_segments, got)
            net.forward_segments_compact(sp_d, ep_d, sv_d, tot, max_segments, want)
        else:
            tv, tv_want = torch.full((cap * 32,), POISON, device="cuda"), torch.full((cap * 32,), POISON, device="cuda")
            net.forward_segments_rays(sp_d, ep_d, sr_d, table, tot, max_segments, got, tv)
            net.forward_segments(sp_d, ep_d, sv_d, tot, max_segments, want, tv_want)
            assert torch.equal(tv, tv_want)
        assert torch.equal(got, want)
        assert bool((got[max_segments * 32:] == POISON).all()) and not bool((got[:max_segments * 32] == POISON).any())


@pytest.mark.gpu
@pytest.mark.parametrize("W,df", VARIANTS)
def test_table_is_the_direction_part_of_layer0(gpu, W, df):
    """Row r of the table against float64: sum over the direction and padding features of W0[row, f] * enc_f(view[r]).
    Bound per element: the kernel's features are fp16 (2^-11 relative on |f| <= 1) of an encoder good to 1e-5 (angle
    doubling, tests/test_gpu_parity.py), the weights are exact fp16 and the fp32 accumulation of <= 64 products adds at most
    64 * 2^-24 relative: (2^-11 + 1e-5 + 64 * 2^-24) * sum |w|."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(W + df)
    n_rays = 77                                                     # 4 full waves of 16 rays and 13 rays: a partial wave, a partial block
    net = _net(torch, api, W, df, 2, seed=5)
    E, width = net.encoded_width(), 2 * (30 + 2 * df)
    w0 = _params(W, 2, E, 5)[:W * E].reshape(W, E).astype(np.float64)
    view = np.stack([rng.uniform(0, 3.1416, n_rays), rng.uniform(-3.1416, 3.1416, n_rays)], axis=1).astype(np.float32)
    table = torch.full((n_rays, W), POISON, device="cuda")
    net.ray_direction_bias(_dev(torch, view), torch.ones(n_rays, dtype=torch.int32, device="cuda"), table)
    got = table.cpu().numpy().astype(np.float64)
    feats = np.ones((n_rays, E - 60))                               # [direction block | padding = 1.0], tcnn Composite order
    for dd in range(2):
        for f in range(df):
            arg = np.pi * 2.0 ** f * view[:, dd].astype(np.float64)
            feats[:, (dd * df + f) * 2], feats[:, (dd * df + f) * 2 + 1] = np.sin(arg), np.cos(arg)
    assert feats.shape[1] == E - 60 and width - 60 == 4 * df
    want = feats @ w0[:, 60:].T
    bound = (2.0 ** -11 + 1e-5 + 64 * 2.0 ** -24) * np.abs(w0[:, 60:]).sum(axis=1)[None, :]
    err = np.abs(got - want)
    print(f"W={W} df={df}: max |table - float64| = {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert np.all(err <= bound), float((err / bound).max())


# ---------------------------------------------------------------------------------------------------- the frame
@pytest.mark.gpu
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("W,depth", [(128, 8), (64, 2), (128, 1), (64, 3)])
def test_frame_equals_the_seg_view_path(gpu, scene, W, depth, compact):
    """render() shades per ray; the slot's radiance (and t_vals) equal the public seg_view entry over the same buffers, the
    slot's seg_ray / table are what the traversal wrote, rays without a hit are never written."""
    torch = gpu
    from rtx_nerf_amd import api
    net = _net(torch, api, W, 12, depth)
    pipe = _pipe(scene, net, compact=compact)
    g = pipe._slots[0]
    assert g.ray_bias is not None and g.seg_ray is not None
    g.ray_bias.fill_(POISON)
    g.radiance.fill_(POISON)
    pipe.set_pose(_pose(30.0))
    pix = pipe.render().clone()
    torch.cuda.synchronize()
    nh, idx, total = g.num_hits.cpu().numpy(), g.indices.cpu().numpy(), int(g.total.item())
    assert total == nh.sum() and total % 16 != 0                    # a last partial tile
    assert (nh == 1).any()                                          # a ray with exactly one segment
    assert ((idx // 16 != (idx + nh - 1) // 16) & (nh > 0)).any()   # rays across a tile boundary
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert (total + 15) // 16 > n_cu - 64                           # blocks with a second tile, one grid stride on
    assert np.array_equal(g.seg_ray[:total].cpu().numpy(), np.repeat(np.arange(nh.size, dtype=np.int32), nh))
    assert torch.equal(g.seg_view[:total], g.view_dirs[g.seg_ray[:total].long()])
    miss = _dev(torch, nh == 0)
    assert bool((g.ray_bias[miss] == POISON).all()) and not bool((g.ray_bias[~miss] == POISON).all(dim=1).any())
    want, tv = _reshade_with_seg_view(torch, pipe, g)
    assert torch.equal(g.radiance, want) and bool((want[total * 32:] == POISON).all())
    if not compact:
        assert torch.equal(g.t_vals[:total * 32], tv[:total * 32])
    assert bool((pix[miss] == 0).all()) and bool((pix[~miss] != 0).any())
    ref = _pipe(scene, net, compact=compact, per_ray=False)          # the whole frame through the per-segment product
    assert ref._slots[0].ray_bias is None and ref._slots[0].seg_ray is None
    ref.set_pose(_pose(30.0))
    assert torch.equal(ref.render(), pix) and torch.equal(ref._slots[0].radiance[:total * 32], g.radiance[:total * 32])


@pytest.mark.gpu
def test_no_segments_at_all(gpu, scene):
    """A pose looking away from the grid: total_segments = 0, no table row and no radiance is written, the frame is black."""
    torch = gpu
    from rtx_nerf_amd import api
    net = _net(torch, api, 128, 12, 2)
    pipe = _pipe(scene, net)
    g = pipe._slots[0]
    g.ray_bias.fill_(POISON)
    g.radiance.fill_(POISON)
    away = _pose(30.0).copy().reshape(4, 4)
    away[:3, :3] = -away[:3, :3]                                    # every ray turned round
    pipe.set_pose(away)
    pix = pipe.render()
    torch.cuda.synchronize()
    assert int(g.total.item()) == 0 and bool((pix == 0).all())
    assert bool((g.ray_bias == POISON).all()) and bool((g.radiance == POISON).all())


@pytest.mark.gpu
def test_capacity_overflow_truncates_as_before(gpu, scene):
    """max_segments below the need: the stored segments are shaded exactly as the seg_view entry shades them and the rays
    that were stored whole are the full frame's pixels; truncated rays are composited over num_stored."""
    torch = gpu
    from rtx_nerf_amd import api
    net = _net(torch, api, 128, 12, 3)
    full = _pipe(scene, net)
    full.set_pose(_pose(30.0))
    want_pix = full.render().clone()
    small = _pipe(scene, net, max_segments=2501, on_overflow="ignore")
    g = small._slots[0]
    g.radiance.fill_(POISON)
    small.set_pose(_pose(30.0))
    pix = small.render().clone()
    torch.cuda.synchronize()
    assert int(g.total.item()) > 2501 and small.overflowed()
    want, _ = _reshade_with_seg_view(torch, small, g)
    assert torch.equal(g.radiance, want) and not bool((want == POISON).any())
    whole = g.num_hits_c == g.num_hits
    assert bool((~whole).any()) and bool((g.num_hits_c[~whole] < g.num_hits[~whole]).all())
    assert torch.equal(pix[whole], want_pix[whole])


@pytest.mark.gpu
def test_a_strided_shard_is_rows_of_the_full_frame(gpu, scene):
    """Rows 1, 4, 7, ... as a windowed shard: seg_ray is the slot-local ray number, so the shard's pixels are the frame's rows."""
    torch = gpu
    from rtx_nerf_amd import api
    from rtx_nerf_amd.shard import RowShard
    net = _net(torch, api, 64, 12, 2)
    full = _pipe(scene, net)
    full.set_pose(_pose(200.0))
    want = full.render().reshape(H_IMG, W_IMG, 3).clone()
    sh = RowShard(W_IMG, H_IMG, 1, 3)
    part = _pipe(scene, net, max_rays=sh.n_local, window=sh.window)
    part.set_pose(_pose(200.0))
    got = part.render(ray_begin=sh.ray_begin, ray_count=sh.n_local).reshape(-1, W_IMG, 3)
    torch.cuda.synchronize()
    assert torch.equal(got, want[1::3]) and bool((got != 0).any())


# ---------------------------------------------------------------------------------------------------- slots
@pytest.mark.gpu
def test_two_slots_in_flight_and_a_slot_reused(gpu, scene):
    """Two poses pipelined on two slots, twice over (the second round re-uses each slot with the OTHER pose): every frame is
    its serial frame.  Then slot 0 serially with a new pose: a fresh pipeline's frame, not the old table's."""
    torch = gpu
    from rtx_nerf_amd import api
    net = _net(torch, api, 128, 12, 2)
    poses = [_pose(30.0), _pose(200.0)]
    ref = _pipe(scene, net)
    want = []
    for p in poses:
        ref.set_pose(p)
        want.append(ref.render().clone())
    assert not torch.equal(want[0], want[1])
    pipe = _pipe(scene, net, n_slots=2)
    poses_d = [_dev(torch, p.reshape(16).astype(np.float32)) for p in poses]
    outs = [torch.empty((W_IMG * H_IMG, 3), device="cuda") for _ in range(4)]
    for i, o in enumerate(outs):
        pipe.render_async(poses_d[(i + i // 2) % 2], out=o)          # 0, 1, 1, 0
    pipe.drain_async()
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert torch.equal(o, want[(i + i // 2) % 2]), f"pipelined frame {i}"
    for k in (0, 1, 0):
        pipe.set_pose(poses[k])
        assert torch.equal(pipe.render(), want[k])


@pytest.mark.gpu
def test_shade_again_reproduces_the_frame(gpu, scene):
    torch = gpu
    from rtx_nerf_amd import api
    net = _net(torch, api, 128, 12, 8)
    pipe = _pipe(scene, net)
    pipe.set_pose(_pose(200.0))
    pipe.render()
    g = pipe._slots[0]
    first = g.radiance.clone()
    g.radiance.fill_(POISON)
    pipe.shade_again(0)
    torch.cuda.synchronize()
    total = int(g.total.item())
    assert total > 0 and torch.equal(g.radiance[:total * 32], first[:total * 32])


@pytest.mark.gpu
def test_captured_frame_follows_the_pose_buffer(gpu, scene):
    """One captured frame replayed three times, the pose buffer rewritten between replays: three eager frames (the table is
    rebuilt inside the graph, from the pose the replay reads)."""
    torch = gpu
    from rtx_nerf_amd import api
    net = _net(torch, api, 64, 12, 3)
    poses = [_pose(30.0), _pose(200.0), _pose(110.0)]
    pipe = _pipe(scene, net)
    want = []
    for p in poses:
        pipe.set_pose(p)
        want.append(pipe.render().clone())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        graph, pix = pipe.capture()
    torch.cuda.synchronize()
    for p, w in zip(poses, want):
        pipe.set_pose(p)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pix, w)
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])


# ---------------------------------------------------------------------------------------------------- the ABI
def test_ray_entries_validate_before_touching_a_device():
    """rtxn_mlp_ray_direction_bias / rtxn_mlp_forward_segments_rays* / rtxn_render_ray_buffers: argument errors are
    RTXN_ERR_INVALID (1) / RTXN_ERR_UNSUPPORTED (3) with a message, with or without a GPU."""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_mlp_ray_direction_bias_supported(None) == 0
    assert lib.rtxn_mlp_ray_direction_bias(None, None, None, 4, None, None) == 1 and b"NULL model" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_forward_segments_rays(None, None, None, None, None, 4, None, 8, C.c_void_p(16), None, None) == 1
    assert lib.rtxn_mlp_forward_segments_rays_compact(None, None, None, None, None, 4, None, 8, C.c_void_p(16), None) == 1
    assert b"NULL model" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_forward_segments_rays(None, None, None, None, None, 4, None, 8, None, None, None) == 1
    assert b"NULL buffer" in lib.rtxn_last_error()
    assert lib.rtxn_render_ray_buffers(None, 0, None, None) == 1 and b"NULL renderer" in lib.rtxn_last_error()
    assert lib.rtxn_render_set_ray_workspace(None, None, 0) == 1 and b"NULL renderer" in lib.rtxn_last_error()
    assert lib.rtxn_render_ray_workspace_bytes(None) == 0 and b"NULL config" in lib.rtxn_last_error()
    h = C.c_void_p()
    for width, supported in ((128, 1), (64, 1), (256, 0)):
        cfg = _lib.MlpConfig(3, 10, 2, 12, width, 2, 4, 1)
        assert lib.rtxn_mlp_create(C.byref(cfg), C.byref(h)) == 0
        assert lib.rtxn_mlp_ray_direction_bias_supported(h) == supported
        rc = lib.rtxn_mlp_ray_direction_bias(h, None, None, 4, None, None)
        rc2 = lib.rtxn_mlp_forward_segments_rays_compact(h, None, None, None, None, 4, None, 8, C.c_void_p(16), None)
        rc_cfg = _lib.RenderConfig()
        rc_cfg.mlp, rc_cfg.width, rc_cfg.height, rc_cfg.grid_res, rc_cfg.trace_mode, rc_cfg.max_segments, rc_cfg.n_slots = h, 64, 48, 32, 1, 1000, 3
        rc_cfg.focal_length, rc_cfg.aspect_ratio = 1.0, 64 / 48
        main = lib.rtxn_render_workspace_bytes(C.byref(rc_cfg))
        ray = lib.rtxn_render_ray_workspace_bytes(C.byref(rc_cfg))
        # per slot int[max_segments] + float[rays][width], each rounded up to 256 bytes; nothing where there is no per-ray kernel
        assert main > 0 and ray == (3 * (4096 + 64 * 48 * width * 4) if supported else 0)
        if supported:                                            # no parameters yet: said before any device is looked for
            assert rc == 1 and rc2 == 1 and b"rtxn_mlp_set_params has not been called" in lib.rtxn_last_error()
        else:
            assert rc == 3 and rc2 == 3 and b"no per-ray kernel" in lib.rtxn_last_error()
        assert lib.rtxn_mlp_destroy(h) == 0


@pytest.mark.gpu
def test_ray_entries_validate_their_sizes_and_alignment(gpu):
    torch = gpu
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    net = _net(torch, api, 64, 12, 1)
    buf = torch.zeros(4096, device="cuda")
    p, ip = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr())
    assert lib.rtxn_mlp_ray_direction_bias(net._h, p, ip, -1, p, None) == 1 and b"n_rays" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_ray_direction_bias(net._h, p, ip, 4, C.c_void_p(buf.data_ptr() + 4), None) == 1
    assert b"16-byte aligned" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_ray_direction_bias(net._h, p, None, 4, p, None) == 1 and b"NULL buffer" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_ray_direction_bias(net._h, None, None, 0, None, None) == 0
    assert lib.rtxn_mlp_forward_segments_rays_compact(net._h, p, p, ip, p, 4, ip, -1, p, None) == 1
    assert b"max_segments" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_forward_segments_rays_compact(net._h, p, p, ip, p, 0, ip, 8, p, None) == 1 and b"n_rays" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_forward_segments_rays_compact(net._h, p, p, None, p, 4, ip, 8, p, None) == 1
    assert b"NULL buffer" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_forward_segments_rays(net._h, p, p, ip, p, 4, ip, 8, C.c_void_p(buf.data_ptr() + 8), None, None) == 1
    assert b"aligned" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_forward_segments_rays_compact(net._h, None, None, None, None, 4, None, 0, None, None) == 0
    wide = api.Network(n_neurons=256, n_hidden_layers=2)
    assert not wide.ray_direction_bias_supported()
