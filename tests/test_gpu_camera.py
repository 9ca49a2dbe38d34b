"""Camera models on the GPU: rtxn_camera_rays against the float64 reference of tests/_camera_float64.py, the batch
draw through cameras against rtxn_draw_batch and rtxn_camera_rays, frames over explicit rays against the per-stage sequence,
Trainer.evaluate over a set with cameras, and the three stepping paths in deterministic mode.

Shapes: frames of 40 x 30 (not square, 1200 pixels: five blocks, the last one partial) for the generator and the draw; a
32 x 24 launch over a 32^3 grid for the frames; the tiny hash model of test_gpu_draw_batch.py on 256 rays for the trainer."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _camera_float64 as F  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N_IMG = F.W, F.H, 3
NPIX = W * H
BAR_D = 2e-6              # the project's bar for generated ray directions against float64, per component
MODEL_NAMES = {F.PINHOLE: "pinhole", F.OPENCV: "opencv", F.OPENCV_FISHEYE: "opencv_fisheye"}
_CACHE = {}


@pytest.fixture(autouse=True)
def _own_timeout():
    """every test here under its own limit: a hung kernel ends the run (with every thread's stack) instead of stalling it"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _poses():
    from rtx_nerf_amd import scenes
    return np.stack([np.asarray(scenes.pose_spherical(35.0 + 110.0 * i, -25.0 - 10.0 * i, origin_scale=10.0), np.float32).reshape(16)
                     for i in range(N_IMG)])


def _cams(model, rows, w=W, h=H):
    from rtx_nerf_amd import api
    return api.camera_set(MODEL_NAMES[model], np.asarray(rows, dtype=np.float32), width=w, height=h)


# ---- 1. the generator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.all_cases(), ids=[c[0] for c in F.all_cases()])
def test_camera_rays_against_float64(gpu, case):
    torch = gpu
    from rtx_nerf_amd import api
    name, model, row = case
    la = _poses()[1]
    la_d = torch.from_numpy(la).cuda()
    cams = _cams(model, row[None])
    o, d = api.camera_rays(cams, 0, la_d, W, H)
    torch.cuda.synchronize()
    o, d = o.cpu().numpy(), d.cpu().numpy()
    o64, d64 = F.camera_rays(model, row, la, W, H)
    err = np.abs(d - d64).max()
    print(f"{name}: max |d - d64| = {err:.3e} (bar {BAR_D:.0e}); max ||d| - 1| = {np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max():.3e}")
    assert err <= BAR_D
    want_o = (la.reshape(4, 4)[:3, 3] / np.float32(10)).astype(np.float32)            # float32 division: IEEE, as the kernel's
    assert want_o.dtype == np.float32 and np.array_equal(o, np.broadcast_to(want_o, o.shape))
    assert np.abs(o - o64).max() <= 1e-7
    # a window: the tail block, and an offset that is no multiple of the wave; only the window's elements change
    begin, count = 37, 301
    po = torch.full((NPIX, 3), -7.0, device="cuda")
    pd = torch.full((NPIX, 3), -7.0, device="cuda")
    api.camera_rays(cams, 0, la_d, W, H, begin, count, po, pd)
    torch.cuda.synchronize()
    po, pd = po.cpu().numpy(), pd.cpu().numpy()
    inside = np.zeros(NPIX, dtype=bool)
    inside[begin:begin + count] = True
    assert np.array_equal(po[inside], o[inside]) and np.array_equal(pd[inside], d[inside])
    assert (po[~inside] == -7).all() and (pd[~inside] == -7).all()


def test_camera_of_a_set_is_selected_by_index(gpu):
    torch = gpu
    from rtx_nerf_amd import _lib, api
    rows = np.stack([F.opencv_params(k) for k in F.OPENCV_SETS[:3]])
    cams = _cams(F.OPENCV, rows)
    la_d = torch.from_numpy(_poses()[0]).cuda()
    for c in range(3):
        _, d = api.camera_rays(cams, c, la_d, W, H)
        _, d1 = api.camera_rays(_cams(F.OPENCV, rows[c:c + 1]), 0, la_d, W, H)
        assert torch.equal(d, d1)
    with pytest.raises(_lib.RtxnError, match=r"camera = 3 out of \[0,3\)"):
        api.camera_rays(cams, 3, la_d, W, H)


# ---- 2., 3. the batch draw ---------------------------------------------------------------------------------------------------
def _frames(torch, channels, u8):
    key = ("frames", channels, u8)
    if key not in _CACHE:
        rng = np.random.default_rng(100 + channels + 10 * u8)
        img = rng.integers(0, 256, (N_IMG, H, W, channels), dtype=np.uint8) if u8 else rng.uniform(0, 1, (N_IMG, H, W, channels)).astype(np.float32)
        _CACHE[key] = (torch.from_numpy(img).cuda(), torch.from_numpy(_poses()).cuda())
    return _CACHE[key]


def _draw(torch, iset, n, seed, step, cameras=None):
    from rtx_nerf_amd import api
    o = torch.full((n + 3, 3), -7.0, device="cuda")
    d = torch.full((n + 3, 3), -7.0, device="cuda")
    t = torch.full((n + 3, iset.channels), -7.0, device="cuda")
    dr = torch.full((n + 3, 2), -7, dtype=torch.int32, device="cuda")
    api.draw_batch(iset, n, seed, torch.full((1,), step, dtype=torch.int32, device="cuda"), o, d, t, dr, cameras=cameras)
    torch.cuda.synchronize()
    for buf in (o, d, t, dr):                   # nothing past ray n - 1 is written (the tail block)
        assert bool((buf[n:] == -7).all())
    return o[:n], d[:n], t[:n], dr[:n]


def test_a_centred_pinhole_set_reproduces_the_rays_of_draw_batch(gpu):
    """fx = fy = focal H / 2, cx = W / 2, cy = H / 2: the pinhole of make_ray; d within the bar, o exactly"""
    torch = gpu
    from rtx_nerf_amd import api, scenes
    focal = scenes.lego_focal_length(True)
    img, poses = _frames(torch, 3, False)
    iset = api.ImageSet(img, poses, focal)
    o, d, _, dr = _draw(torch, iset, 1000, 7, 5)
    cams = _cams(F.PINHOLE, F.params(fx=focal * H / 2, fy=focal * H / 2, cx=W / 2, cy=H / 2)[None])
    dr = dr.cpu().numpy()
    worst = 0.0
    for i in range(N_IMG):
        co, cd = api.camera_rays(cams, 0, poses[i], W, H)
        m = dr[:, 0] == i
        assert m.sum() > 200
        worst = max(worst, float((d[m] - cd[dr[m, 1]]).abs().max()))
        assert torch.equal(o[m], co[dr[m, 1]])
    print(f"max |d(draw_batch) - d(centred pinhole camera)| = {worst:.3e} (bar {BAR_D:.0e})")
    assert worst <= BAR_D


def _camera_rows(kind):
    model, n = kind
    if model == F.PINHOLE:
        return np.stack([F.params(fx=F.FX + 2 * i, cx=F.CX - i) for i in range(n)])
    if model == F.OPENCV:
        return np.stack([F.opencv_params(F.OPENCV_SETS[(i + 1) % 4], fx=F.FX + i, cy=F.CY - i) for i in range(n)])
    return np.stack([F.fisheye_params(F.FISHEYE_SETS[i % 3], fy=F.FY + i, cx=F.CX + i) for i in range(n)])


@pytest.mark.parametrize("kind", [(F.OPENCV, 1), (F.OPENCV, 3), (F.OPENCV_FISHEYE, 3), (F.PINHOLE, 1)],
                         ids=["opencv-shared", "opencv-per-image", "fisheye-per-image", "pinhole-shared"])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_draw_batch_cameras(gpu, kind, channels, u8):
    torch = gpu
    from rtx_nerf_amd import api, scenes
    n, seed, step = 300, 7, 5
    img, poses = _frames(torch, channels, u8)
    plain = api.ImageSet(img, poses, scenes.lego_focal_length(True))
    rows = _camera_rows(kind)
    cams = _cams(kind[0], rows)
    iset = api.ImageSet(img, poses, cameras=cams)                  # no focal length: it is not read
    _, d0, t0, dr0 = _draw(torch, plain, n, seed, step)
    o, d, t, dr = _draw(torch, iset, n, seed, step)
    assert torch.equal(dr, dr0) and torch.equal(t, t0), "the same (image, pixel) and the same target bits as rtxn_draw_batch"
    if kind[0] != F.PINHOLE:
        assert not torch.equal(d, d0)
    drn = dr.cpu().numpy()
    assert len(set(drn[:, 0].tolist())) == N_IMG
    for i in range(N_IMG):
        co, cd = api.camera_rays(cams, iset.camera_of(i), poses[i], W, H)
        m = torch.from_numpy(drn[:, 0] == i).cuda()
        pix = dr[m, 1].long()
        assert torch.equal(o[m], co[pix]) and torch.equal(d[m], cd[pix]), f"image {i}: not the rays of rtxn_camera_rays, bit for bit"
    # cameras= given explicitly over a set without any draws the same batch
    o2, d2, t2, dr2 = _draw(torch, plain, n, seed, step, cameras=cams)
    assert torch.equal(o2, o) and torch.equal(d2, d) and torch.equal(t2, t) and torch.equal(dr2, dr)
    if kind[1] == N_IMG:
        assert not np.array_equal(rows[0], rows[1])                 # per-image parameters do differ


# ---- 4. frames over explicit rays ----------------------------------------------------------------------------------------------
FR, FW, FH = 32, 32, 24
FN = FW * FH


def _frame_setup(torch, model):
    """(pipeline, rays_o, rays_d, origin) made once per model: a 32 x 24 launch over a 32^3 grid occupied inside a ball of radius 1.2 (cut by the cube),
    rays of an OPENCV camera from rtxn_camera_rays"""
    key = ("frame", model)
    if key in _CACHE:
        return _CACHE[key]
    from rtx_nerf_amd import api, render, scenes
    dense = scenes.sphere_density(FR, 1.2)
    occ = torch.from_numpy(scenes.pack_occupancy(dense).view(np.int32).copy()).cuda()
    kw = dict(occupancy=occ, aux=True, max_segments=FN * 40)
    if model == "hash":
        hg = api.HashGrid(8, 2, 14, 8, 1.6, n_dir_freqs=4)
        E = hg.encoded_width()
        net = api.Network(n_neurons=64, n_hidden_layers=3, n_encoded_features=E)
        net.set_params(torch.from_numpy(scenes.xavier_params_fp16(64, 3, E, seed=5)).cuda())
        table = torch.from_numpy(np.random.default_rng(5).uniform(-0.5, 0.5, hg.n_params()).astype(np.float16)).cuda()
        pipe = render.RenderPipeline(net, FR, FW, FH, 1.0, vr_mode=api.VR_NERF, step_scale=40.0, hashgrid=hg, table=table, **kw)
    else:
        net = api.Network(n_neurons=64, n_hidden_layers=2)
        net.set_params(torch.from_numpy(scenes.xavier_params_fp16(64, 2, 112, seed=1337)).cuda())
        pipe = render.RenderPipeline(net, FR, FW, FH, 1.0, **kw)
    s = FW / W
    row = F.opencv_params(F.OPENCV_SETS[2], fx=F.FX * s, fy=F.FY * s, cx=F.CX * s, cy=F.CY * s)
    cams = _cams(F.OPENCV, row[None], FW, FH)
    la = np.asarray(scenes.pose_spherical(30.0, -30.0, origin_scale=10.0), np.float32).reshape(16)
    o, d = api.camera_rays(cams, 0, torch.from_numpy(la).cuda(), FW, FH)
    torch.cuda.synchronize()
    _CACHE[key] = (pipe, o, d, la.reshape(4, 4)[:3, 3] / 10.0, cams, torch.from_numpy(la).cuda())
    return _CACHE[key]


def _frame(torch, pipe, o, d, begin=0, count=None, **kw):
    res = pipe.render_rays(o, d, begin, count, depth=True, opacity=True, **kw)
    out = tuple(t.clone() for t in res)
    torch.cuda.synchronize()
    return out


def _stage_sequence(torch, pipe, o, d):
    """the frame through the stage entry points of api: trace with explicit rays -> [per-ray direction product] -> scan -> trace
    write -> fused forward -> compositor, in buffers of this function's own"""
    from rtx_nerf_amd import api
    occ, K = pipe.occ, api.NUM_SAMPLES_PER_SEGMENT
    coarse, bricks = api.build_occupancy_mip(occ, FR), api.build_occupancy_bricks(occ, FR)
    sup = api.build_occupancy_mip(coarse, FR // 4)
    Q = pipe.sub_rays
    nh = torch.zeros(FN, dtype=torch.int32, device="cuda")
    vd = torch.zeros((FN, 2), device="cuda")
    sub = torch.zeros(FN * max(Q, 1), dtype=torch.int32, device="cuda")
    kw = dict(grid_res=FR, rays_o=o, rays_d=d, width=FW, height=FH, ray_begin=0, ray_count=FN, occupancy=occ, occupancy_coarse=coarse,
              occupancy_bricks=bricks, occupancy_super=sup, mode=api.TRACE_DDA, viewing_direction=vd, num_hits=nh, sub_rays=Q, sub_hits=sub)
    api.trace_grid(None, **kw)
    per_ray = pipe.hg is None and pipe.ray_bias is not None
    if per_ray:
        bias = torch.zeros((FN, pipe.net.cfg.n_neurons), device="cuda")
        pipe.net.ray_direction_bias(vd, nh, bias)
    idx, total = api.scan_hits(nh)
    P = int(total.item())
    assert 100 < P <= pipe.max_segments
    sp, ep = torch.zeros((P, 3), device="cuda"), torch.zeros((P, 3), device="cuda")
    sv, ts, te = torch.zeros((P, 2), device="cuda"), torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
    sr = torch.zeros(P, dtype=torch.int32, device="cuda")
    ns = torch.zeros(FN, dtype=torch.int32, device="cuda")
    api.trace_grid(None, indices=idx, start_points=sp, end_points=ep, seg_view=sv, t_start=ts, t_end=te, num_stored=ns, segment_capacity=P,
                   **(dict(seg_ray=sr) if per_ray else {}), **kw)
    rad = torch.zeros((P * K, 4), dtype=torch.float16, device="cuda")
    pix, dep, acc = torch.zeros((FN, 3), device="cuda"), torch.zeros(FN, device="cuda"), torch.zeros(FN, device="cuda")
    if pipe.hg is not None:
        step = torch.zeros(P, device="cuda")
        api.hashmlp_forward_segments(pipe.net, pipe.hg, pipe.table, sp, ep, sv, total, P, rad, pipe.sample_type, pipe.step_scale, step)
        hit = step
    else:
        if per_ray:
            pipe.net.forward_segments_rays(sp, ep, sr, bias, total, P, rad)
        else:
            pipe.net.forward_segments_compact(sp, ep, sv, total, P, rad)
        hit = None
    api.volrender_fwd_aux(rad, hit, ns, idx, FN, K, pix, mode=pipe.vr_mode, sample_type=pipe.sample_type, t_start=ts, t_end=te, depth=dep,
                          opacity=acc)
    torch.cuda.synchronize()
    return (pix, dep, acc), nh, P


@pytest.mark.parametrize("model", ["hash", "freq"])
def test_frame_over_rays_equals_the_stage_sequence(gpu, model):
    torch = gpu
    pipe, o, d, *_ = _frame_setup(torch, model)
    got = _frame(torch, pipe, o, d)
    want, nh, P = _stage_sequence(torch, pipe, o, d)
    for name, g, w in zip(("pixels", "depth", "opacity"), got, want):
        assert torch.equal(g, w), f"{name}: {int((g != w).sum())} of {g.numel()} differ"
    assert float(got[0].abs().max()) > 0 and float(got[2].max()) > 0.1 and bool((got[2][nh == 0] == 0).all())
    assert not pipe.overflowed()
    # the counting entry: the sum of num_hits of the count pass
    assert pipe.count_segments_rays(o, d) == int(nh.sum().item()) == P
    assert pipe.count_segments_rays(o, d, 100, 200) == int(nh[100:300].sum().item())
    # pixels alone (the plain compositor) and a background
    only = pipe.render_rays(o, d)
    assert only[1] is None and only[2] is None and torch.equal(only[0], got[0])
    bg = _frame(torch, pipe, o, d, background=(0.25, 1.0, 0.0))
    assert torch.equal(bg[2], got[2]) and torch.equal(bg[0][:, 2], got[0][:, 2]) and not torch.equal(bg[0][:, 1], got[0][:, 1])


@pytest.mark.parametrize("model", ["hash", "freq"])
def test_a_half_window_is_that_slice_of_the_frame(gpu, model):
    torch = gpu
    pipe, o, d, *_ = _frame_setup(torch, model)
    full = _frame(torch, pipe, o, d)
    half = _frame(torch, pipe, o, d, FN // 2, FN // 2)
    first = _frame(torch, pipe, o, d, 0, FN // 2 - 7)
    for f, h, a in zip(full, half, first):
        assert torch.equal(h, f[FN // 2:]) and torch.equal(a, f[:FN // 2 - 7])


@pytest.mark.parametrize("model", ["hash", "freq"])
def test_a_captured_frame_over_rays_equals_the_eager_one(gpu, model):
    torch = gpu
    pipe, o, d, _, cams, la = _frame_setup(torch, model)
    eager = _frame(torch, pipe, o, d)
    via_camera = tuple(t.clone() for t in pipe.render_camera(cams, 0, la, depth=True, opacity=True))     # also allocates the pipeline's rays
    out = (torch.zeros((FN, 3), device="cuda"), torch.zeros(FN, device="cuda"), torch.zeros(FN, device="cuda"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pipe.render_camera(cams, 0, la, depth=True, opacity=True, out=out)
    g.replay()
    torch.cuda.synchronize()
    for e, v, c in zip(eager, via_camera, out):
        assert torch.equal(e, v) and torch.equal(e, c)
    # the replay follows the pose: another pose in the same buffer, replayed, equals that pose eagerly
    from rtx_nerf_amd import scenes
    la.copy_(torch.from_numpy(np.asarray(scenes.pose_spherical(75.0, -20.0, origin_scale=10.0), np.float32).reshape(16)).cuda())
    g.replay()
    torch.cuda.synchronize()
    moved = tuple(t.clone() for t in out)
    again = tuple(t.clone() for t in pipe.render_camera(cams, 0, la, depth=True, opacity=True))
    torch.cuda.synchronize()
    for m, a, e in zip(moved, again, eager):
        assert torch.equal(m, a) and not torch.equal(m, e)
    la.copy_(torch.from_numpy(np.asarray(scenes.pose_spherical(30.0, -30.0, origin_scale=10.0), np.float32).reshape(16)).cuda())
    torch.cuda.synchronize()


@pytest.mark.parametrize("model,eps", [("hash", 0.22), ("freq", 0.27)])
def test_termination_over_rays_stays_within_the_threshold(gpu, model, eps):
    """the bound of tests/test_gpu_render_termination.py (test_the_bound): pixels and opacity move by at most eps, depth by at most
    eps x the largest sample distance, each plus twice the compositor bar of 1e-5; opacity only ever drops"""
    torch = gpu
    BAR = 1e-5
    pipe, o, d, origin, *_ = _frame_setup(torch, model)
    plain = [t.cpu().numpy().astype(np.float64) for t in _frame(torch, pipe, o, d, background=(0.25, 1.0, 0.0))]
    total = int(pipe.total.item())
    t_max = float(np.linalg.norm(pipe.end[:total].cpu().numpy().astype(np.float64) - origin[None, :], axis=1).max())
    nh = pipe.num_hits_c.clone()
    pipe.set_termination(eps, 2, 2)
    try:
        got = [t.cpu().numpy().astype(np.float64) for t in _frame(torch, pipe, o, d, background=(0.25, 1.0, 0.0))]
        shaded = pipe.shaded_per_ray().clone()
    finally:
        pipe.set_termination(None)
    d_pix, d_acc, d_dep = np.abs(got[0] - plain[0]), plain[2] - got[2], np.abs(got[1] - plain[1])
    print(f"{model}: eps {eps}: max |pixel| {d_pix.max():.3e}, opacity {d_acc.min():.3e} .. {d_acc.max():.3e}, |depth| / t_max "
          f"{d_dep.max() / t_max:.3e}; rays cut short: {int((shaded < nh).sum())} of {int((nh > 0).sum())}")
    assert (d_pix <= eps + 2 * BAR).all()
    assert (0 <= d_acc + 2 * BAR).all() and (d_acc <= eps + 2 * BAR).all()
    assert (d_dep <= eps * t_max + 2 * BAR * t_max).all()
    assert bool((shaded <= nh).all())
    # cleared again: the plain frame bit for bit
    back = _frame(torch, pipe, o, d, background=(0.25, 1.0, 0.0))
    assert np.array_equal(back[0].cpu().numpy().astype(np.float64), plain[0])


# ---- 5. evaluation ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int64)


def test_evaluate_renders_each_frame_with_its_camera(gpu):
    torch = gpu
    from rtx_nerf_amd import api, scenes
    from rtx_nerf_amd.train import Trainer, camera_rays
    R, B = 16, 900
    hgd = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()
    tr = Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=4, hashgrid=hgd, n_dir_freqs=4, batch_rays=B, max_segments=B * 30,
                 lr=1e-2, loss_scale=128.0, density_scale=120.0, mode="nerf", seed=3)
    for i in range(3):
        o, d = camera_rays(scenes.pose_spherical(40.0 + 50.0 * i, -30.0 + 5.0 * i, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
        tr.step(o, d, torch.from_numpy(np.random.default_rng(i).uniform(0, 1, (B, 3)).astype(np.float32)).cuda())
    frames = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (3, FH, FW, 3), dtype=np.uint8)).cuda()
    poses = torch.from_numpy(np.stack([scenes.pose_spherical(30.0 + 70.0 * i, -25.0 - 10.0 * i, origin_scale=10.0) for i in range(3)])
                             .astype(np.float32)).cuda()
    s = FW / W
    rows = np.stack([F.opencv_params(F.OPENCV_SETS[i + 1], fx=(F.FX + i) * s, fy=F.FY * s, cx=F.CX * s, cy=(F.CY - i) * s) for i in range(3)])
    cams = _cams(F.OPENCV, rows, FW, FH)
    iset = api.ImageSet(frames, poses, cameras=cams)
    rec = tr.evaluate(iset).clone()
    assert rec.shape == (3, 3) and bool(torch.isfinite(rec).all())
    pipe = tr.render_pipeline(FW, FH, 1.0, max_segments=FN * 40)
    rows_want = []
    for i in range(3):
        frame = pipe.render_camera(cams, i, iset.poses[i])[0].clone()
        assert float(frame.abs().max()) > 0
        rows_want.append(api.image_metrics(iset, i, frame))
    torch.cuda.synchronize()
    assert not pipe.overflowed()
    assert np.array_equal(_bits(rec), _bits(torch.stack(rows_want))), (rec, rows_want)
    # the same frames and poses under the centred pinhole nearest to the cameras: other rays, other rows
    plain = tr.evaluate(api.ImageSet(frames, poses, 2.0 * F.FX * s / FH))
    assert not np.array_equal(_bits(plain[:, 0]), _bits(rec[:, 0]))
    assert len(tr._eval_pipelines) == 2
    assert np.array_equal(_bits(tr.evaluate(iset, images=[2, 0])), _bits(rec[[2, 0]]))
    # replayed from a graph: the same rows
    out = torch.zeros((3, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.evaluate(iset, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(rec))
    assert len(tr._eval_pipelines) == 2


# ---- 6. the three stepping paths, deterministic ------------------------------------------------------------------------------------
def test_stepping_paths_draw_through_the_cameras_bit_for_bit(gpu):
    """RTXN_DETERMINISTIC=1 in a fresh child process (tests/_camera_paths_child.py): step_images, capture_step(draw=True) with and
    without prefetch, step_entry and a trainer fed the same batches by hand end every step with identical parameters"""
    env = dict(os.environ, RTXN_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_camera_paths_child.py")], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=170)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("CAMERA_PATHS ")][-1]
    out = json.loads(line[len("CAMERA_PATHS "):])
    want = out["by_hand"]
    assert len(want) == 3 and len(set(want)) == 3
    for path in ("step_images", "captured", "captured_prefetch", "step_entry"):
        assert out[path] == want, f"{path}: parameters differ from the trainer fed by hand: {out[path]} vs {want}"
    assert out["by_hand_without_cameras"][0] != want[0]              # the cameras do change the rays the model is trained on
    assert len(out["drawn"]) == 256
