"""Depth, opacity and background (rtxn_volrender_fwd_aux, RenderPipeline(aux=True).render_ex / render_async_ex / capture_ex):
the standalone compositor against a float64 restatement, its pixels against the plain compositors bit for bit, and whole
frames against a restatement built from the slot buffers and the camera origin."""
import numpy as np
import pytest

from rtx_nerf_amd import scenes

pytestmark = pytest.mark.gpu
K32 = 32


# ------------------------------------------------------------------------------------------ float64 restatement
def _restate(rad, nh, idx, K, mode, t_hit, dist):
    """rad float64[N, 4]; t_hit: per-sample float64[N] (COMPAT: the t_vals; NERF: step lengths); dist: per-sample distance
    float64[N] or None.  Returns pixels[B, 3], opacity[B], depth[B] (as rtxn_volrender_fwd_aux defines them)."""
    B = len(nh)
    pix, acc, dep = np.zeros((B, 3)), np.zeros(B), np.zeros(B)
    for r in range(B):
        a, n = int(idx[r]) * K, int(nh[r]) * K
        if n == 0:
            continue
        c, t = rad[a:a + n], t_hit[a:a + n]
        if mode == 0:   # COMPAT: delta across the whole ray (t_{-1} = 0), inclusive optical depth
            delta = np.abs(t - np.concatenate([[0.0], t[:-1]]))
            x = delta * c[:, 3]
            w = np.exp(-np.cumsum(x)) * (1 - np.exp(-x))
        else:
            x = t * c[:, 3]
            w = np.exp(-(np.cumsum(x) - x)) * (1 - np.exp(-x))
        pix[r] = (w[:, None] * c[:, :3]).sum(0)
        acc[r] = w.sum()
        if dist is not None:
            dep[r] = (w * dist[a:a + n]).sum()
    return pix, acc, dep


def _sample_u(K, sample_type):
    return (np.arange(K) + (0.5 if sample_type == 3 else 0.0)) / K


# ------------------------------------------------------------------------------------------ standalone compositor
def _synthetic(rng, B, K, sparse):
    nh = rng.integers(0, 9, B).astype(np.int32)
    nh[::7] = 0
    nh[1::11] = 12                                          # 12 x 32 = 384 samples: carries across three 128-sample steps
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
    P = int(nh.sum())
    N = P * K
    rad = rng.uniform(0, 1, (N, 4)).astype(np.float32)
    if sparse:
        sig = np.where(rng.uniform(0, 1, N) < 0.05, rng.uniform(5, 80, N), 0.0)
    else:
        sig = rng.uniform(0, 40, N)
    rad[:, 3] = sig
    rad16 = rad.astype(np.float16)
    t_vals = rng.uniform(0.001, 0.1, N).astype(np.float32)            # COMPAT float4: any t sequence
    steps = rng.uniform(0.001, 0.06, N).astype(np.float32)            # NERF float4: per-sample step lengths
    seg_step = rng.uniform(0.001, 0.06, P).astype(np.float32)         # NERF half4: one step per segment
    ts = rng.uniform(2.0, 6.0, P).astype(np.float32)
    te = (ts + rng.uniform(0.0, 0.2, P)).astype(np.float32)
    return dict(nh=nh, idx=idx, P=P, N=N, rad=rad, rad16=rad16, t_vals=t_vals, steps=steps, seg_step=seg_step, ts=ts, te=te)


CASES = [  # layout, vr_mode, sample_type, K, sparse, B
    ("half4", 0, 0, 32, False, 37),
    ("half4", 0, 0, 32, True, 1001),
    ("half4", 1, 3, 32, False, 37),
    ("half4", 1, 3, 32, True, 1001),
    ("half4", 1, 0, 32, False, 130),
    ("float4", 0, 0, 32, False, 37),
    ("float4", 0, 3, 32, True, 1001),
    ("float4", 1, 3, 32, False, 130),
    ("float4", 1, 0, 32, True, 37),
    ("half4", 0, 0, 7, False, 37),         # odd K: the one-sample kernels
    ("half4", 1, 3, 7, True, 37),
    ("float4", 0, 0, 7, True, 37),
    ("float4", 1, 3, 7, False, 37),
    ("half4-misaligned", 1, 3, 32, False, 37),   # 8- but not 16-byte aligned half4 radiance: the one-sample kernel
    ("half4-misaligned", 0, 0, 32, True, 37),
]


@pytest.mark.parametrize("layout,mode,stype,K,sparse,B", CASES)
def test_aux_compositor_matches_float64_and_the_plain_compositor(gpu, layout, mode, stype, K, sparse, B):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(CASES.index((layout, mode, stype, K, sparse, B)))
    s = _synthetic(rng, B, K, sparse)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    nh_d, idx_d, ts_d, te_d = dev(s["nh"]), dev(s["idx"]), dev(s["ts"]), dev(s["te"])
    N, P = s["N"], s["P"]
    kk = np.tile(np.arange(K), P)
    if layout.startswith("half4"):
        if layout == "half4-misaligned":
            buf = torch.zeros((N + 1, 4), dtype=torch.float16, device="cuda")
            buf[1:] = dev(s["rad16"])
            rad_d = buf[1:]
            assert rad_d.data_ptr() % 16 == 8
        else:
            rad_d = dev(s["rad16"])
        rad = s["rad16"].astype(np.float64)
        if mode == 0:
            hit_d, t_hit = None, (kk + 1) / K                         # implicit REGULAR t_vals
        else:
            hit_d, t_hit = dev(s["seg_step"]), np.repeat(s["seg_step"].astype(np.float64), K)
    else:
        rad_d, rad = dev(s["rad"]), s["rad"].astype(np.float64)
        h = s["t_vals"] if mode == 0 else s["steps"]
        hit_d, t_hit = dev(h), h.astype(np.float64)
    u = np.tile(_sample_u(K, stype), P)
    ts64, te64 = np.repeat(s["ts"].astype(np.float64), K), np.repeat(s["te"].astype(np.float64), K)
    dist = ts64 + u * (te64 - ts64)
    want_pix, want_acc, want_dep = _restate(rad, s["nh"], s["idx"], K, mode, t_hit, dist)

    pix0 = torch.full((B, 3), float("nan"), device="cuda")
    dep = torch.full((B,), float("nan"), device="cuda")
    acc = torch.full((B,), float("nan"), device="cuda")
    api.volrender_fwd_aux(rad_d, hit_d, nh_d, idx_d, B, K, pix0, mode=mode, sample_type=stype, t_start=ts_d, t_end=te_d,
                          depth=dep, opacity=acc)
    # the plain compositor of the same layout
    plain = torch.full((B, 3), float("nan"), device="cuda")
    if layout.startswith("half4"):
        if mode == 0:
            api.volrender_compact(rad_d, nh_d, idx_d, B, K, plain)
        else:
            api.volrender_compact_nerf(rad_d, hit_d, nh_d, idx_d, B, K, plain)
    else:
        api.launch_volrender_cuda(None, rad_d, nh_d, idx_d, hit_d, B, K, plain, mode)
    bg = (0.25, 1.0, 0.0)
    pix_bg = torch.full((B, 3), float("nan"), device="cuda")
    acc_bg = torch.full((B,), float("nan"), device="cuda")
    api.volrender_fwd_aux(rad_d, hit_d, nh_d, idx_d, B, K, pix_bg, mode=mode, sample_type=stype, opacity=acc_bg, background=bg)
    torch.cuda.synchronize()

    assert torch.equal(pix0, plain), "with no background the pixels must be the plain compositor's bit for bit"
    p0, a, d = pix0.cpu().numpy(), acc.cpu().numpy(), dep.cpu().numpy()
    np.testing.assert_allclose(p0, want_pix, rtol=0, atol=1e-5)
    np.testing.assert_allclose(a, want_acc, rtol=0, atol=1e-5)
    np.testing.assert_allclose(d, want_dep, rtol=0, atol=1e-5 * float(s["te"].max()))
    # fp32 rounding of a sum of weights that telescopes to 1 - exp(-T) can land an ulp or two above 1 on opaque rays
    assert (a >= 0).all() and (a <= 1 + 1e-6).all()
    assert torch.equal(acc_bg, acc)
    pb = pix_bg.cpu().numpy()
    np.testing.assert_allclose(pb - p0, (1 - a)[:, None] * np.array(bg)[None, :], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(pb[:, 2], p0[:, 2])                  # a zero channel of the background is left alone
    empty = s["nh"] == 0
    assert empty.any()
    assert (a[empty] == 0).all() and (d[empty] == 0).all() and (p0[empty] == 0).all()
    np.testing.assert_array_equal(pb[empty], np.tile(np.array(bg, dtype=np.float32), (int(empty.sum()), 1)))
    if mode == 0:
        # COMPAT's inclusive optical depth takes each sample's own absorption out of its weight: a dense ray's opacity
        # saturates well below 1 (the reference's quirk, kept), so only check that the inputs are not trivially transparent
        assert (a[~empty] > 0.01).any()
    elif sparse:
        assert (a > 0.5).any() and (a[~empty] < 0.5).any()
    else:
        assert (a[s["nh"] >= 4] > 0.99).all()


def test_aux_closed_form_constant_density(gpu):
    """One segment of constant density in NERF mode: w_i = q^i (1 - q), q = exp(-x), so opacity = 1 - q^K and depth follows
    from the geometric series sum_i q^i (1 - q) (a + b i) with a = t0 + u0 L / K, b = L / K."""
    torch = gpu
    from rtx_nerf_amd import api
    K = K32
    for sigma, step, t0, L, stype in ((3.0, 0.05, 2.5, 1.6, 3), (20.0, 0.01, 4.0, 0.32, 3), (0.5, 0.02, 1.0, 0.64, 0)):
        rad = np.zeros((K, 4), np.float16)
        rad[:, :3] = 0.5
        rad[:, 3] = sigma
        out = torch.empty((1, 3), device="cuda")
        dep, acc = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        one = lambda v, dt: torch.tensor([v], dtype=dt, device="cuda")
        api.volrender_fwd_aux(torch.from_numpy(rad).cuda(), one(step, torch.float32), one(1, torch.int32), one(0, torch.int32),
                              1, K, out, mode=1, sample_type=stype, t_start=one(t0, torch.float32),
                              t_end=one(t0 + L, torch.float32), depth=dep, opacity=acc)
        torch.cuda.synchronize()
        s = float(np.float32(step))
        q = np.exp(-s * float(np.float16(sigma)))
        a, b = t0 + (0.5 if stype == 3 else 0.0) * L / K, L / K
        geo = (1 - q ** K) / (1 - q)
        igeo = q * (1 - K * q ** (K - 1) + (K - 1) * q ** K) / (1 - q) ** 2
        want_acc = 1 - q ** K
        want_dep = (1 - q) * (a * geo + b * igeo)
        assert abs(float(acc.item()) - want_acc) < 1e-5
        assert abs(float(dep.item()) - want_dep) < 1e-5 * (t0 + L)
        assert abs(float(out[0, 0].item()) - 0.5 * want_acc) < 1e-5


# ------------------------------------------------------------------------------------------ whole frames
def _freq_net(torch, api):
    params = scenes.xavier_params_fp16(64, 2, 112, seed=1337)
    net = api.Network(n_neurons=64, n_hidden_layers=2)
    net.set_params(torch.from_numpy(params).cuda())
    return net


def _hash_model(torch, api, seed=5):
    hg = api.HashGrid(8, 2, 14, 8, 1.6, n_dir_freqs=4)
    E = hg.encoded_width()
    net = api.Network(n_neurons=64, n_hidden_layers=3, n_encoded_features=E)
    net.set_params(torch.from_numpy(scenes.xavier_params_fp16(64, 3, E, seed=seed)).cuda())
    table = np.random.default_rng(seed).uniform(-0.5, 0.5, hg.n_params()).astype(np.float16)
    return hg, net, torch.from_numpy(table).cuda()


SETUPS = ["freq-compact-compat", "freq-float4-nerf", "hash-compact-nerf"]
R, W, H = 32, 48, 40


def _pipeline(torch, setup, **kw):
    from rtx_nerf_amd import api, render
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.7)).view(np.int32).copy()).cuda()
    f = scenes.lego_focal_length(True)
    kw.setdefault("max_segments", W * H * 40)
    if setup == "freq-compact-compat":
        return render.RenderPipeline(_freq_net(torch, api), R, W, H, f, occupancy=occ, aux=True, **kw)
    if setup == "freq-float4-nerf":
        return render.RenderPipeline(_freq_net(torch, api), R, W, H, f, occupancy=occ, vr_mode=api.VR_NERF, aux=True, **kw)
    hg, net, table = _hash_model(torch, api)
    p = render.RenderPipeline(net, R, W, H, f, occupancy=occ, vr_mode=api.VR_NERF, step_scale=40.0, hashgrid=hg, table=table,
                              aux=True, **kw)
    p._keep = (hg, net, table)
    return p


POSES = [scenes.pose_spherical(30.0, -30.0, origin_scale=10.0), scenes.pose_spherical(75.0, -20.0, origin_scale=10.0),
         scenes.pose_spherical(150.0, -45.0, origin_scale=10.0), scenes.pose_spherical(-60.0, -10.0, origin_scale=10.0)]


def _frame_restatement(pipe, look_at, n):
    """float64 restatement of a frame's opacity and depth from slot 0's buffers and the camera origin (make_ray: the
    look_at translation / 10); distances are computed from the segment end points, not from the kernel's t_start."""
    K = K32
    nh = pipe.num_hits_c[:n].cpu().numpy()
    idx = pipe.indices[:n].cpu().numpy()
    P = int(nh.sum())
    top = int((idx + nh)[nh > 0].max())            # past the last stored segment (truncated rays' indices may run beyond)
    start = pipe.start[:top].cpu().numpy().astype(np.float64)
    end = pipe.end[:top].cpu().numpy().astype(np.float64)
    rad = pipe.radiance[:top * K].float().cpu().numpy().astype(np.float64)
    if pipe.compact:
        t_hit = (np.tile(np.arange(K), top) + 1) / K if pipe.vr_mode == 0 else np.repeat(pipe.seg_step[:top].cpu().numpy(), K)
    else:
        t_hit = pipe.t_vals[:top * K].cpu().numpy()
    la = np.asarray(look_at, np.float32).reshape(16)
    o = np.array([la[3] / np.float32(10), la[7] / np.float32(10), la[11] / np.float32(10)], np.float64)
    u = np.tile(_sample_u(K, pipe.sample_type), top)
    p = np.repeat(start, K, axis=0) + u[:, None] * (np.repeat(end, K, axis=0) - np.repeat(start, K, axis=0))
    dist = np.linalg.norm(p - o[None, :], axis=1)
    pix, acc, dep = _restate(rad, nh, idx, K, pipe.vr_mode, t_hit.astype(np.float64), dist)
    return pix, acc, dep, P, float(np.linalg.norm(end - o[None, :], axis=1).max())


@pytest.mark.parametrize("setup", SETUPS)
def test_render_ex_matches_render_and_the_restatement(gpu, setup):
    torch = gpu
    pipe = _pipeline(torch, setup)
    for la in POSES[:2]:
        pipe.set_pose(la)
        plain = pipe.render().clone()
        pix, dep, acc = pipe.render_ex()
        pix, dep, acc = pix.clone(), dep.clone(), acc.clone()
        pix2, dep2, acc2 = pipe.render_ex()
        torch.cuda.synchronize()
        assert not pipe.overflowed()
        assert torch.equal(pix, plain), "render_ex without a background must give render()'s pixels bit for bit"
        assert torch.equal(pix2, pix) and torch.equal(dep2, dep) and torch.equal(acc2, acc), "two runs differ"
        want_pix, want_acc, want_dep, P, tmax = _frame_restatement(pipe, la, pipe.max_rays)
        assert P > 200
        a, d = acc.cpu().numpy(), dep.cpu().numpy()
        np.testing.assert_allclose(a, want_acc, rtol=0, atol=1e-5)
        np.testing.assert_allclose(d, want_dep, rtol=0, atol=1e-5 * tmax)
        # the restatement's pixels: the slot buffers and the weights are right (half radiance is exact in float64)
        np.testing.assert_allclose(pix.cpu().numpy(), want_pix, rtol=0, atol=1e-5)
        assert (a >= 0).all() and (a <= 1 + 1e-6).all() and (a > 0.05).any()
        hit = a > 1e-3
        surf = d[hit] / a[hit]                                         # expected termination distance of the hit rays
        assert (surf > 0).all() and (surf < tmax + 1e-4).all()
        # background: pixels + (1 - opacity) bg; opacity and depth unchanged; only what was asked for is written
        bg = (1.0, 0.5, 0.25)
        pbg, dnone, abg = pipe.render_ex(background=bg, depth=False)
        torch.cuda.synchronize()
        assert dnone is None and torch.equal(abg, acc)
        np.testing.assert_allclose((pbg - pix).cpu().numpy(), (1 - a)[:, None] * np.array(bg)[None, :], rtol=0, atol=1e-6)


def test_depth_needs_the_aux_flag(gpu):
    torch = gpu
    import ctypes as C
    from rtx_nerf_amd import _lib, api, render
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.7)).view(np.int32).copy()).cuda()
    pipe = render.RenderPipeline(_freq_net(torch, api), R, W, H, scenes.lego_focal_length(True), occupancy=occ,
                                 max_segments=W * H * 40)
    pipe.set_pose(POSES[0])
    with pytest.raises(ValueError):
        pipe.render_ex()
    o = _lib.RenderOutputs()
    o.pixels, o.depth = C.c_void_p(pipe.pixels.data_ptr()), C.c_void_p(pipe.opacity.data_ptr())
    assert _lib.lib().rtxn_render_frame_ex(pipe._h, 0, C.c_void_p(pipe.look_at.data_ptr()), 0, 0, C.byref(o), api._stream()) == 1
    assert b"RTXN_RENDER_AUX" in _lib.lib().rtxn_last_error()
    # opacity and the background work without the flag
    plain = pipe.render().clone()
    pix, dep, acc = pipe.render_ex(depth=False)
    torch.cuda.synchronize()
    assert dep is None and torch.equal(pix, plain) and float(acc.max()) > 0.05


@pytest.mark.parametrize("setup,n_slots,host", [("freq-compact-compat", 2, False), ("freq-float4-nerf", 3, True),
                                                ("hash-compact-nerf", 3, False), ("hash-compact-nerf", 2, True)])
def test_render_async_ex_equals_serial(gpu, setup, n_slots, host):
    torch = gpu
    pipe = _pipeline(torch, setup, n_slots=n_slots)
    bg = (0.0, 1.0, 0.5)
    want = []
    for la in POSES:
        pipe.set_pose(la)
        want.append(tuple(t.clone() for t in pipe.render_ex(background=bg)))
    torch.cuda.synchronize()
    n = pipe.max_rays
    outs = []
    for k in range(2 * len(POSES)):                                     # more frames than slots
        la = POSES[k % len(POSES)]
        o = (torch.empty((n, 3), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda"))
        pose = la.reshape(16).astype(np.float32) if host else torch.from_numpy(la.reshape(16).astype(np.float32)).cuda()
        pix, dep, acc, comp = pipe.render_async_ex(pose, background=bg, out=o)
        outs.append((pose, o))
    pipe.finish()
    for k, (_, o) in enumerate(outs):
        w = want[k % len(POSES)]
        for got, exp in zip(o, w):
            assert torch.equal(got, exp), f"frame {k}"


@pytest.mark.parametrize("setup", ["freq-compact-compat", "hash-compact-nerf"])
def test_captured_render_ex_replays_with_a_new_pose(gpu, setup):
    torch = gpu
    pipe = _pipeline(torch, setup)
    bg = (0.2, 0.3, 0.4)
    pipe.set_pose(POSES[0])
    pipe.render_ex(background=bg)
    torch.cuda.synchronize()
    g, pix, dep, acc = pipe.capture_ex(background=bg)
    for la in POSES[1:3]:
        pipe.set_pose(la)
        g.replay()
        got = (pix.clone(), dep.clone(), acc.clone())
        eager = tuple(t.clone() for t in pipe.render_ex(background=bg))
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert torch.equal(a, b)
    assert not pipe.overflowed()


@pytest.mark.parametrize("setup", ["freq-compact-compat", "hash-compact-nerf"])
def test_overflow_keeps_depth_and_opacity_consistent_with_the_truncated_pixels(gpu, setup):
    torch = gpu
    pipe = _pipeline(torch, setup, max_segments=300, on_overflow="ignore")
    pipe.set_pose(POSES[0])
    plain = pipe.render().clone()
    pix, dep, acc = (t.clone() for t in pipe.render_ex())
    torch.cuda.synchronize()
    assert pipe.overflowed()
    nh, ns = pipe.num_hits.cpu().numpy(), pipe.num_hits_c.cpu().numpy()
    assert (ns < nh).any() and int(ns.sum()) <= 300
    assert torch.equal(pix, plain)
    want_pix, want_acc, want_dep, P, tmax = _frame_restatement(pipe, POSES[0], pipe.max_rays)
    np.testing.assert_allclose(pix.cpu().numpy(), want_pix, rtol=0, atol=1e-5)
    np.testing.assert_allclose(acc.cpu().numpy(), want_acc, rtol=0, atol=1e-5)
    np.testing.assert_allclose(dep.cpu().numpy(), want_dep, rtol=0, atol=1e-5 * tmax)
    a = acc.cpu().numpy()
    assert (a[ns == 0] == 0).all() and (dep.cpu().numpy()[ns == 0] == 0).all()


def test_windowed_shard_matches_the_full_frame(gpu):
    torch = gpu
    full = _pipeline(torch, "hash-compact-nerf")
    full.set_pose(POSES[1])
    fp, fd, fa = (t.clone() for t in full.render_ex(background=(1.0, 1.0, 1.0)))
    n_local = W * H // 2
    shard = _pipeline(torch, "hash-compact-nerf", window=(W, 2 * W), max_rays=n_local)
    shard.set_pose(POSES[1])
    sp, sd, sa = shard.render_ex(ray_begin=W, ray_count=n_local, background=(1.0, 1.0, 1.0))   # the odd image rows
    torch.cuda.synchronize()
    rows = np.arange(n_local)
    gid = torch.from_numpy(W + (rows // W) * 2 * W + rows % W).cuda()
    for a, b in ((sp, fp[gid]), (sd, fd[gid]), (sa, fa[gid])):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=1e-6)
    assert float(sa.max()) > 0.05
