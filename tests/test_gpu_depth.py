"""Depth supervision on the GPU (include/rtxn.h, rtxn_train_depth, rtxn_depth_targets): the DEPTH instantiations of
the training compositor (composite_train.hip) against the float64 restatement and bound of tests/_depth_float64.py; an inactive
struct is the rung below bit for bit; the fixed-order loss sum of deterministic mode; the depth-target kernel against its float64
conversion; agreement of the eager / captured / one-call steps; and end-to-end training of the few-view sphere teacher.

Measured values: profiles/r25/depth_tests.txt."""
import faulthandler
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _compositor_float64 as c64  # noqa: E402
import _depth_float64 as d64  # noqa: E402

LS, LAMBDA_Z = 128.0, 1.0          # tests/test_depth_float64_reference.py: the term is visible through fp16 at these
LAMBDA_D, LAMBDA_A = 10.0, 0.5     # the "everything active" case: tests/test_gpu_distortion.py's weights
COLOR = (0.9, 0.25, 1.0)
U = 2.0 ** -24
SCHEDULE = {32: "pair", 7: "one"}


@pytest.fixture(autouse=True)
def _own_timeout():
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(torch, **arrays):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}


def _scaler(torch, api, scale):
    cfg = api.loss_scaler(init_scale=scale)
    state, ws = api.loss_scaler_state_tensor(cfg), api.loss_scaler_workspace()
    return api.loss_scaler(cfg.init_scale, cfg.growth, cfg.backoff, cfg.growth_interval, cfg.min_scale, cfg.max_scale, cfg.max_grad_norm,
                           state=state, partials=ws)


def _inputs(K, t_scale=1.0):
    """the batch of _depth_float64.batch(K) as the compositor reads it; t_scale != 1: as a trainer with that density_scale hands it
    over (step lengths times it, sigma divided by it, the distances untouched)"""
    b, z = d64.batch(K)
    rad, step = b.rad, b.step
    if t_scale != 1.0:
        rad = rad.copy()
        rad[:, 3] /= np.float32(t_scale)
        step = step * np.float32(t_scale)
    return b, z, rad, step


def _run(torch, api, K, kind, *, weight=LAMBDA_Z, full=False, misaligned=False, scaled=False, t_scale=1.0, outputs=True, term=True):
    """one compositor call.  full: Huber colour loss, the alpha term, a constant background with RGBA targets and the distortion
    regulariser beside the depth term; term=False: the call without the depth struct (the rung below), everything else the same;
    term="empty": a struct with weight 0 and nothing else in it"""
    b, z, rad, step = _inputs(K, t_scale)
    B = b.B
    dev = _dev(torch, rad=rad, step=step, nh=b.nh, idx=b.idx, tgt=b.tgt if full else b.tgt[:, :3], ts=b.ts, te=b.te, z=z)
    if misaligned:
        dev["step"] = torch.cat([torch.zeros(1, device="cuda"), dev["step"]])[1:]
        assert dev["step"].data_ptr() % 8 == 4 and dev["step"].is_contiguous()
    new = lambda: torch.full((B,), -1.0, device="cuda")
    opa = new() if full else None
    dist, dep_reg = (new(), new()) if full else (None, None)
    bg = api.train_background(COLOR, target_channels=4) if full else None
    spec = api.train_loss("huber", opacity_weight=LAMBDA_A, opacity=opa) if full else None
    reg = api.train_regularizer(LAMBDA_D, dev["ts"], dev["te"], dist, dep_reg) if full else None
    D, lz = (new(), new()) if outputs else (None, None)
    depth = (api.train_depth(0.0) if term == "empty" else
             api.train_depth(weight, kind, None, dev["z"], dev["ts"], dev["te"], D, lz) if term else None)
    sc = _scaler(torch, api, LS) if scaled else None
    pix = torch.zeros((B, 3), device="cuda")
    lg = torch.zeros((B, 3), dtype=torch.float16, device="cuda")
    loss = torch.full((1,), 9.0, device="cuda")           # a stale value: the call must replace it
    out = torch.full((b.N + c64.TAIL, 4), c64.SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16)     # an fp16 NaN pattern
    api.volrender_depth_train(dev["rad"], dev["step"], dev["nh"], dev["idx"], B, K, dev["tgt"], LS, pix, lg, loss, out, bg, spec, reg, sc, depth)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in
            dict(pix=pix, lg=lg, loss=loss, out=out, opa=opa, dist=dist, dep_reg=dep_reg, D=D, lz=lz).items()}


def _check(torch, K, kind, *, full=False, misaligned=False, scaled=False, t_scale=1.0):
    """Every output of one call against float64: pixels (3e-6, the loss tests' bar), D_r (the derived dD, and
    tests/test_gpu_distortion.py's 3e-6 max m), v l(e) per ray (d64.loss_bar), the scalar, every radiance-gradient element within
    d64.gradients' bound, the tail untouched; and a ray without a target has the gradients of the call without the term."""
    from rtx_nerf_amd import api
    b, z, rad, step = _inputs(K, t_scale)
    B = b.B
    got = _run(torch, api, K, kind, full=full, misaligned=misaligned, scaled=scaled, t_scale=t_scale)
    below = _run(torch, api, K, kind, full=full, misaligned=misaligned, scaled=scaled, t_scale=t_scale, term=False)
    bt = b._replace(rad=rad, step=step)
    bg = np.tile(np.array(COLOR, np.float32), (B, 1)) if full else None
    alpha = b.tgt[:, 3].astype(np.float64)
    gA = None
    if full:            # g_A recomputed from the kernel's own A by the kernel's operations (fp32, then fp16)
        inv_rays = np.float32(1.0) / np.float32(B)
        gA = (np.float32(LS) * (np.float32(LAMBDA_A) * (np.float32(2.0) * (got["opa"] - b.tgt[:, 3]))) * inv_rays).astype(np.float16).astype(np.float64)
    kz = d64.k_factor(LS, LAMBDA_Z, B)
    kd = d64.k_factor(LS, LAMBDA_D, B) if full else 0.0
    res = d64.gradients(bt, z, got["lg"].astype(np.float64), "one" if misaligned else SCHEDULE[K], kind, kz, bg=bg, gA=gA, reg_k=kd)
    have = got["out"]
    c64.check_written(have, b.N)
    # (with t_scale sigma is the batch's, 1 / t_scale of the world's: its gradient and its bound, which carry the step length, follow)
    table = c64.check_elements(f"depth {kind} K={K}", have[:b.N], res.ref, res.bound, bt)
    m, _ = c64.midpoints(b)
    m_max = np.array([m[s].max() if s.stop > s.start else 0.0 for s in c64.ray_slices(b)])
    hit = b.nh > 0
    D_err = np.abs(got["D"] - res.D)
    D_ratio, D_bar = (D_err[hit] / res.dD[hit]).max(), (D_err[hit] / (3e-6 * m_max[hit])).max()
    lz_ratio = (np.abs(got["lz"] - res.lz) / np.maximum(d64.loss_bar(kind, res, z), 1e-300))[d64.valid(z)].max()
    pix_err = np.abs(got["pix"] - res.pix).max()
    # the scalar from the kernel's own stored pixels, opacities, L_r and D_r in float64: what is left is the fp32 rounding of a ray's
    # share (at most 12 operations on the colour + alpha part, 3 on either other share, their sums 2) and of the sum itself (a
    # float atomic per block of four rays, or per ray: at most B additions), every term positive: (B + 30) u relative
    tg = c64.composited_target(bg, b.tgt) if full else b.tgt[:, :3].astype(np.float64)
    e = got["pix"].astype(np.float64) - tg
    l, _ = c64.loss_terms("huber" if full else "l2", e, got["pix"].astype(np.float64), 0.1)
    zz = np.where(d64.valid(z), np.nan_to_num(z.astype(np.float64)), 0.0)
    lzk, _ = d64.loss_terms(kind, got["D"].astype(np.float64) - zz)
    parts = [float(l.sum() / (3 * B)), LAMBDA_Z / B * float(np.where(d64.valid(z), lzk, 0.0).sum())]
    if full:
        parts += [float(np.float32(LAMBDA_A)) / B * float(((got["opa"].astype(np.float64) - alpha) ** 2).sum()),
                  LAMBDA_D / B * float(got["dist"].astype(np.float64).sum())]
    loss_err = abs(float(got["loss"][0]) - sum(parts)) / sum(parts)
    none = ~d64.valid(z)
    per_sample = np.repeat(none, b.nh.astype(np.int64) * K)
    print(f"\n[{kind} K={K}{' full' if full else ''}{' misaligned' if misaligned else ''}{' scaled' if scaled else ''} t_scale={t_scale}] pixels max|err| {pix_err:.2e}  "
          f"D_r err / dD {D_ratio:.3f}, / (3e-6 max m) {D_bar:.3f}  l(e) err / bar {lz_ratio:.3f}  loss {sum(parts):.5f} (depth share "
          f"{parts[1]:.5f}) rel {loss_err:.2e} (bar {(B + 30) * U:.2e})  depth addend moves {d64.moved_share(res, z, bt):.3f} of the sigma-gradients")
    print("\n".join(c64.table_lines(f"depth {kind} K={K}", table)))
    np.testing.assert_allclose(got["pix"], res.pix, rtol=0, atol=3e-6)
    assert D_ratio <= 1.0 and D_bar <= 1.0
    assert np.all(got["D"][~hit] == 0.0)
    assert lz_ratio <= 1.0 and np.all(got["lz"][none] == 0.0)
    assert min(parts) > 1e-3 and loss_err <= (B + 30) * U
    # without a target: the values of the call without the term (a zero may change its sign: the addend is + 0.0); with one: not
    assert np.array_equal(have[:b.N][per_sample].astype(np.float32), below["out"][:b.N][per_sample].astype(np.float32))
    assert not np.array_equal(have[:b.N][~per_sample], below["out"][:b.N][~per_sample])
    assert np.array_equal(got["pix"], below["pix"]) and np.array_equal(got["lg"].view(np.uint16), below["lg"].view(np.uint16))
    if full:
        assert np.array_equal(got["dep_reg"], got["D"])
    return got, res


@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("kind", d64.KINDS)
def test_depth_compositor_against_float64(gpu, kind, K):
    """K = 32: composite_train_multi_kernel<true, 4, false, true>, 17 and 40 segments cross its 512-sample step; K = 7:
    composite_train_kernel<true, false, true>, 10 segments cross its 64-sample step.  301 rays, every segment count of
    {0, 1, 2, 3, 10, 17, 40}, a quarter without a target (zeros, one negative, one NaN).  lambda_z = 1, loss scale 128."""
    _check(gpu, K, kind)


@pytest.mark.parametrize("K", [32, 7])
def test_depth_compositor_with_every_other_term_active(gpu, K):
    """Huber colour loss, the alpha term, a constant background with RGBA targets and the distortion regulariser (lambda_d = 10)
    beside a Huber depth term"""
    _check(gpu, K, "huber", full=True)


def test_misaligned_step_lengths_take_the_one_ray_kernel_at_an_even_K(gpu):
    """K = 32 with the step lengths 4 bytes off an 8-byte boundary: composite_train_kernel<true, false, true>, held to the one-ray
    schedule's bound"""
    _check(gpu, 32, "l2", misaligned=True)


@pytest.mark.parametrize("K", [32, 7])
def test_depth_compositor_reading_the_loss_scale_from_the_scaler(gpu, K):
    """the DEV instantiations: k_z formed on the device from the scaler's word, by the host's expression"""
    a, _ = _check(gpu, K, "l2", scaled=True)
    from rtx_nerf_amd import api
    b = _run(gpu, api, K, "l2")
    for k in ("pix", "lg", "out", "D", "lz"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k       # the same scale by either route: the same bits


@pytest.mark.parametrize("K", [32, 7])
def test_step_lengths_with_a_density_scale_leave_the_distances_alone(gpu, K):
    """The batch of a trainer with density_scale 120: D_r comes from t_start / t_end, not from the step lengths -- every bar holds
    against the same float64 D_r, and D_r is the unscaled call's to its own bound"""
    a, res = _check(gpu, K, "l2", t_scale=120.0)
    from rtx_nerf_amd import api
    b = _run(gpu, api, K, "l2")
    assert np.all(np.abs(a["D"] - b["D"]) <= 2 * res.dD + 1e-300) and a["D"].max() > 1.0


def test_inactive_struct_is_the_rung_below_bit_for_bit_on_the_compositor(gpu):
    """depth None, weight 0 without outputs (with or without buffers): bitwise rtxn_volrender_reg_train / _scaled_train, the scalar
    included, in deterministic mode"""
    torch = gpu
    from rtx_nerf_amd import api
    shadow = api.deterministic_shadow(64)
    api.set_deterministic(shadow, None)
    try:
        for K in (32, 7):
            for full in (False, True):
                ref = _run(torch, api, K, "l2", full=full, term=False)
                for form in ("empty", "zero_buffers"):
                    got = _run(torch, api, K, "l2", full=full, weight=0.0, outputs=False, term="empty" if form == "empty" else True)
                    for k in ("pix", "lg", "out", "loss", "opa", "dist"):
                        if ref[k] is not None:
                            assert np.array_equal(ref[k].view(np.uint8), got[k].view(np.uint8)), (K, full, form, k)
                assert float(np.nanmax(np.abs(ref["out"][:-c64.TAIL].astype(np.float32)))) > 0.0
    finally:
        api.set_deterministic(None, None)


def _fixed_order(pix, tgt, D, z, weight):
    """rtxn's fixed-order sum restated in fp32, operation for operation, for L2 colour and an L2 depth term without a background:
    per ray ((e0^2 + e1^2 + e2^2) * (1 / (3 n))) + (weight * (D - z)^2) * (1 / n) on rays with a target; groups of four as
    (a + b) + (c + d); one group per thread of 1024 (n <= 4096); a halving tree over the threads."""
    f = np.float32
    B = pix.shape[0]
    inv_n, inv_rays = f(1.0) / f(3 * B), f(1.0) / f(B)
    e = pix - tgt
    sq = e * e
    v = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) * inv_n
    ez = D - np.where(d64.valid(z), z, f(0.0))
    lz = np.where(d64.valid(z), ez * ez, f(0.0)).astype(np.float32)
    v = v + (f(weight) * lz) * inv_rays
    assert v.dtype == np.float32
    g = np.zeros(4 * ((B + 3) // 4), np.float32)
    g[:B] = v
    g = g.reshape(-1, 4)
    red = np.zeros(1024, np.float32)
    red[:g.shape[0]] = (g[:, 0] + g[:, 1]) + (g[:, 2] + g[:, 3])
    n = 512
    while n:
        red[:n] = red[:n] + red[n:2 * n]
        n //= 2
    return red[0]


@pytest.mark.parametrize("K", [32, 7])
def test_deterministic_loss_scalar_is_the_fixed_order_sum(gpu, K):
    torch = gpu
    from rtx_nerf_amd import api
    api.set_deterministic(None, None)
    default = _run(torch, api, K, "l2")
    shadow = api.deterministic_shadow(64)
    api.set_deterministic(shadow, None)
    try:
        det, det2 = _run(torch, api, K, "l2"), _run(torch, api, K, "l2")
        with pytest.raises(api._lib.RtxnError, match="depth->depth"):       # the term is summed from the D_r stored there
            _run(torch, api, K, "l2", outputs=False)
    finally:
        api.set_deterministic(None, None)
    for k in ("pix", "lg", "out", "D", "lz"):               # everything but the scalar is the default mode's, bit for bit
        assert np.array_equal(default[k].view(np.uint8), det[k].view(np.uint8)), k
        assert np.array_equal(det[k].view(np.uint8), det2[k].view(np.uint8)), k
    b, z = d64.batch(K)
    want = _fixed_order(det["pix"], b.tgt[:, :3], det["D"], z, LAMBDA_Z)
    print(f"\n[K={K}] deterministic {det['loss'][0]:.9e}, fp32 restatement {want:.9e}, default mode {default['loss'][0]:.9e}")
    assert det["loss"][0] == want == det2["loss"][0] and want > 1e-3


# ---- rtxn_depth_targets ------------------------------------------------------------------------------------------------------------
def _target_set(torch, api, fmt, kind, cameras):
    """3 images of 5 x 4; depth values in millimetres of the poses' unit, zeros sprinkled in (f32: also a NaN, a negative value and
    an Inf); cameras: one wide opencv camera for all three"""
    from rtx_nerf_amd import scenes
    rng = np.random.default_rng(17)
    N, H, W = 3, 4, 5
    frames = rng.uniform(0, 1, (N, H, W, 3)).astype(np.float32)
    poses = np.stack([np.asarray(scenes.pose_spherical(35.0 + 110.0 * i, -25.0 - 10.0 * i, origin_scale=10.0), np.float32).reshape(16) for i in range(N)])
    v = rng.integers(20000, 60000, (N, H, W)).astype(np.uint16)
    v.reshape(-1)[::7] = 0
    depth = v if fmt == "u16" else (v.astype(np.float32) * np.float32(1.0009765625))
    if fmt == "f32":
        depth.reshape(-1)[3], depth.reshape(-1)[5], depth.reshape(-1)[11] = np.float32(np.nan), np.float32(-4.0), np.float32(np.inf)
    cams = None
    if cameras:
        cams = api.camera_set("opencv", np.asarray([api.camera_params(4.1, 3.9, 2.4, 2.1, k1=0.05, k2=-0.01, p1=0.002, p2=-0.001)], np.float32), W, H)
    iset = api.ImageSet(torch.from_numpy(frames).cuda(), torch.from_numpy(poses).cuda(), scenes.lego_focal_length(True), cameras=cams,
                        depth=torch.from_numpy(depth).cuda(), depth_unit=1e-3, depth_kind=kind)
    return iset, depth, poses


@pytest.mark.parametrize("cameras", [False, True])
@pytest.mark.parametrize("kind", ["z", "ray"])
@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_depth_targets_against_float64(gpu, fmt, kind, cameras):
    """every pixel of a 3-image set of 5 x 4 frames drawn (several times over), through the pinhole and one opencv camera (a wide
    one: off-axis cosines down to ~0.8): each target within _depth_float64.target_u(cond) half-ulps-at-worst of the float64
    conversion, zeros where the map has no value"""
    torch = gpu
    from rtx_nerf_amd import api
    iset, depth, poses = _target_set(torch, api, fmt, kind, cameras)
    n = 600
    o, d, t = torch.zeros((n, 3), device="cuda"), torch.zeros((n, 3), device="cuda"), torch.zeros((n, 3), device="cuda")
    drawn = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    z = torch.full((n,), -1.0, device="cuda")
    api.draw_batch(iset, n, 5, None, o, d, t, drawn)
    api.depth_targets(iset, n, drawn, d, z)
    torch.cuda.synchronize()
    dr, dn, got = drawn.cpu().numpy(), d.cpu().numpy(), z.cpu().numpy()
    assert len({(int(a), int(b)) for a, b in dr}) == 60          # every pixel of every image
    v = depth.reshape(3, -1)[dr[:, 0], dr[:, 1]]
    scale = np.float32(1e-3) * np.float32(0.1)
    want, cond, c = d64.depth_targets(v, scale, kind, dn, poses, dr[:, 0])
    bar = (d64.target_u(cond) if kind == "z" else d64.TARGET_U_RAY) * U * np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    print(f"\n[{fmt} {kind} cameras={cameras}] {int((want > 0).sum())} targets of {n}, cosine {c.min():.3f} .. {c.max():.3f}, "
          f"max err / bar {(err / np.maximum(bar, 1e-300))[want > 0].max():.3f}")
    assert (want > 0).sum() > n // 2 and (want == 0).sum() > 20
    assert np.all(got[want == 0] == 0.0) and np.all(err <= bar)
    if kind == "z":
        assert np.all(got[want > 0] >= (v.astype(np.float64) * float(scale))[want > 0] * (1 - 4 * U))      # a distance along the ray >= z


def test_depth_targets_of_a_grazing_ray_and_of_a_pixel_outside_the_set(gpu):
    """rays handed over by the caller: cosines either side of 2^-6 against pose column 2, one looking backwards; a drawn record that
    names no pixel of the set.  No target for c <= 2^-6, and nothing is read out of bounds."""
    torch = gpu
    from rtx_nerf_amd import api
    iset, depth, poses = _target_set(torch, api, "u16", "z", False)
    l = poses[1].reshape(4, 4)[:3, 2].astype(np.float64)
    f = -l / np.linalg.norm(l)
    side = np.cross(f, [0.3, 0.2, 0.9]); side /= np.linalg.norm(side)
    cosines = [1.0, 0.5, 2.0 ** -5, 2.0 ** -7, 0.0, -0.5]
    d = np.stack([c * f + np.sqrt(1 - c * c) * side for c in cosines] + [f, f]).astype(np.float32)
    drawn = np.array([[1, 6]] * len(cosines) + [[3, 0], [0, 20]], np.int32)        # image 3 and pixel 20 do not exist
    assert depth[1].reshape(-1)[6] > 0
    z = torch.full((8,), -1.0, device="cuda")
    api.depth_targets(iset, 8, torch.from_numpy(drawn).cuda(), torch.from_numpy(d).cuda(), z)
    torch.cuda.synchronize()
    got = z.cpu().numpy()
    t = float(np.float32(depth[1].reshape(-1)[6]) * (np.float32(1e-3) * np.float32(0.1)))
    assert np.all(got[3:] == 0.0) and np.all(got[:3] > 0.0), got
    # the directions are rounded to float32 before the kernel sees them: 2^-24 against a cosine of 2^-5 is 2e-6 on its own
    np.testing.assert_allclose(got[:3], [t / c for c in cosines[:3]], rtol=2e-5)


def test_depth_targets_read_the_live_poses(gpu):
    """after a pose step the targets are those of the refined poses, bit for bit: the kernel reads ImageSet.poses where they lie"""
    torch = gpu
    from rtx_nerf_amd import api
    iset, depth, poses = _target_set(torch, api, "u16", "z", False)
    n = 200
    o, d, t = (torch.zeros((n, 3), device="cuda") for _ in range(3))
    drawn = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    api.draw_batch(iset, n, 9, None, o, d, t, drawn)
    z0, z1, z2 = (torch.zeros(n, device="cuda") for _ in range(3))
    api.depth_targets(iset, n, drawn, d, z0)
    N = 3
    delta = torch.zeros((N, 6), device="cuda")
    grad = torch.zeros((N, 8), device="cuda")
    grad[:, :6] = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (N, 6)).astype(np.float32)).cuda()
    grad[:, 6] = 5.0                                            # every image has rays
    pose = api.pose_refinement(N, lr=0.05, poses0=iset.poses.clone(), poses=iset.poses, delta=delta, m=torch.zeros((N, 6), device="cuda"),
                               v=torch.zeros((N, 6), device="cuda"), steps=torch.zeros(N, dtype=torch.int32, device="cuda"), grad=grad)
    api.pose_step(pose)
    api.depth_targets(iset, n, drawn, d, z1)                    # the same rays against the moved optical axes
    twin = api.ImageSet(iset.images, iset.poses.clone(), iset.focal_length, depth=iset.depth, depth_unit=1e-3, depth_kind="z")
    api.depth_targets(twin, n, drawn, d, z2)
    torch.cuda.synchronize()
    assert float(delta.abs().max()) > 0.0
    assert torch.equal(z1, z2) and not torch.equal(z0, z1)


# ---- the three stepping paths --------------------------------------------------------------------------------------------------
STEP_LAMBDA, STEP_LS = 0.5, 128.0


def _sphere_occ(torch, R):
    from rtx_nerf_amd import scenes
    return torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()


def _small_trainer(torch, encoding, seed=3, **kw):
    """tests/test_gpu_distortion.py's _small_trainer"""
    from rtx_nerf_amd.train import Trainer
    R, B = 16, 900
    hgd = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
    kw.setdefault("loss_scale", STEP_LS)
    return Trainer(R, _sphere_occ(torch, R), encoding=encoding, n_neurons=64, n_hidden_layers=4 if encoding == "hash" else 2,
                   hashgrid=hgd if encoding == "hash" else None, n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2,
                   density_scale=120.0, mode="nerf", seed=seed, **kw)


_BATCHES = {}


def _batches(torch, n):
    """(rays_o, rays_d, colour targets, depth targets 3 .. 5 world units, every fifth ray without one)"""
    if n not in _BATCHES:
        from rtx_nerf_amd import scenes
        from rtx_nerf_amd.train import camera_rays
        focal = scenes.lego_focal_length(True)
        rng = np.random.default_rng(8)
        out = []
        for i in range(n):
            o, d = camera_rays(scenes.pose_spherical(25.0 + 55.0 * i, -28.0 + 4.0 * i, origin_scale=10.0), focal, 30, 30)
            z = rng.uniform(3.0, 5.0, 900).astype(np.float32)
            z[::5] = 0.0
            out.append((o, d, torch.from_numpy(rng.uniform(0, 1, (900, 3)).astype(np.float32)).cuda(), torch.from_numpy(z).cuda()))
        _BATCHES[n] = out
    return _BATCHES[n]


def _image_set(torch):
    from rtx_nerf_amd import api, scenes
    rng = np.random.default_rng(5)
    frames = rng.uniform(0, 1, (3, 24, 24, 3)).astype(np.float32)
    poses = np.stack([np.asarray(scenes.pose_spherical(35.0 + 110.0 * i, -25.0 - 10.0 * i, origin_scale=10.0), np.float32).reshape(16)
                      for i in range(3)])
    depth = rng.integers(30000, 50000, (3, 24, 24)).astype(np.uint16)
    depth.reshape(-1)[::5] = 0
    return api.ImageSet(torch.from_numpy(frames).cuda(), torch.from_numpy(poses).cuda(), scenes.lego_focal_length(True),
                        depth=torch.from_numpy(depth).cuda(), depth_unit=1e-3, depth_kind="z")


def _fill(tr, o, d, t, z):
    tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t); tr.graph_depth_targets.copy_(z)


@pytest.mark.parametrize("encoding,jitter,kind", [("hash", False, "l2"), ("hash", True, "huber"), ("freq", True, "l1"), ("freq", False, "l2")])
def test_eager_captured_and_one_call_steps_agree(gpu, encoding, jitter, kind):
    """step(..., depth_targets), step_captured() and step_entry() over graph_depth_targets with depth_weight > 0, deterministic
    mode: the same loss scalar, D_r, l(e_r) and parameters after each of three steps, bit for bit.  A trainer without the term
    ends elsewhere."""
    torch = gpu
    kw = dict(deterministic=True, sample_jitter=jitter, jitter_seed=11, depth_weight=STEP_LAMBDA, depth_loss=kind)
    a, b, c = (_small_trainer(torch, encoding, **kw) for _ in range(3))
    b.capture_step(900, launch_segments=900 * 30)
    c.entry_args(900, launch_segments=900 * 30)
    for i, (o, d, t, z) in enumerate(_batches(torch, 3)):
        la = a.step(o, d, t, z).clone()
        Da, lza = a.depth.clone(), a.depth_loss.clone()
        _fill(b, o, d, t, z)
        lb = b.step_captured().clone()
        Db, lzb = b.depth.clone(), b.depth_loss.clone()
        _fill(c, o, d, t, z)
        lc = c.step_entry().clone()
        torch.cuda.synchronize()
        assert float(Da.max()) > 0.0 and float(lza.max()) > 0.0 and float(la) > 0.0
        assert float(lza[::5].abs().max()) == 0.0                   # the rays without a target
        for name, x, lx, Dx, lzx in (("captured", b, lb, Db, lzb), ("one-call", c, lc, c.depth, c.depth_loss)):
            assert torch.equal(Da, Dx) and torch.equal(lza, lzx), (name, i)
            assert torch.equal(la, lx), (name, i, float(la), float(lx))
            assert torch.equal(a.params, x.params) and torch.equal(a.master, x.master), (name, i)
    assert a.step_count == b.step_count == c.step_count == 3
    plain = _small_trainer(torch, encoding, deterministic=True, sample_jitter=jitter, jitter_seed=11)
    assert plain.depth is None and plain.t_start is None and plain._depth is None and plain.depth_targets is None
    for o, d, t, z in _batches(torch, 3):
        plain.step(o, d, t)
    assert not torch.equal(plain.master, a.master)


@pytest.mark.parametrize("encoding", ["hash", "freq"])
def test_drawn_batches_eager_captured_and_one_call_agree(gpu, encoding):
    """attach_images() over a set with depth maps: step_images(), capture_step(draw=True) -- the target kernel is the graph's
    second node -- and entry_args(draw=True) / step_entry(), deterministic mode, bit for bit: the drawn pixels, the depth
    targets, D_r, the loss and the parameters"""
    torch = gpu
    iset = _image_set(torch)
    kw = dict(deterministic=True, depth_weight=STEP_LAMBDA)
    a, b, c = (_small_trainer(torch, encoding, **kw).attach_images(iset) for _ in range(3))
    b.capture_step(900, launch_segments=900 * 30, draw=True)
    c.entry_args(900, launch_segments=900 * 30, draw=True)
    for i in range(3):
        la = a.step_images().clone()
        lb = b.step_captured().clone()
        lc = c.step_entry().clone()
        torch.cuda.synchronize()
        assert float(la) > 0 and float(a.depth_targets.max()) > 3.0 and float((a.depth_targets == 0).sum()) > 100
        for name, x, lx in (("captured", b, lb), ("one-call", c, lc)):
            assert torch.equal(a.drawn[:900], x.drawn[:900]), (name, i)
            assert torch.equal(a.depth_targets, x.depth_targets) and torch.equal(a.depth, x.depth), (name, i)
            assert torch.equal(la, lx), (name, i, float(la), float(lx))
            assert torch.equal(a.master, x.master), (name, i)
    assert a.draw_count == b.draw_count == c.draw_count == 3
    with pytest.raises(ValueError, match="depth maps"):
        from rtx_nerf_amd import api
        _small_trainer(torch, encoding, depth_weight=STEP_LAMBDA).attach_images(api.ImageSet(iset.images, iset.poses, iset.focal_length))


def test_prefetched_drawn_captured_steps_agree_with_eager(gpu):
    """capture_step(prefetch=True, draw=True): batch k + 1 is drawn and traversed into the second buffer set -- with a target buffer
    and a depth struct of its own -- beside the gradient kernels of batch k.  Deterministic mode: the losses, one call later, and
    the parameters after flush_captured() are the eager trainer's bit for bit; five batches, so both sets train."""
    torch = gpu
    iset = _image_set(torch)
    kw = dict(deterministic=True, depth_weight=STEP_LAMBDA)
    a, b = (_small_trainer(torch, "hash", **kw).attach_images(iset) for _ in range(2))
    b.capture_step(900, launch_segments=900 * 30, prefetch=True, draw=True)
    assert len(b._g_sets) == 2 and b._g_sets[1]["depth"] is not b._g_sets[0]["depth"]
    assert b._g_sets[1]["depth_targets"].data_ptr() != b.depth_targets.data_ptr()
    eager = [a.step_images().clone() for _ in range(5)]
    got = []
    for _ in range(5):
        r = b.step_captured()
        got.append(None if r is None else r.clone())
    assert got[0] is None and b.step_count == 4
    got = got[1:] + [b.flush_captured().clone()]
    torch.cuda.synchronize()
    assert b.step_count == 5 and b.truncated_steps == 0
    for i, (x, y) in enumerate(zip(eager, got)):
        assert float(x) > 0.0 and torch.equal(x, y), (i, float(x), float(y))
    assert torch.equal(a.master, b.master) and torch.equal(a.depth, b.depth)
    assert float(b._g_sets[1]["depth_targets"].max()) > 3.0


@pytest.mark.parametrize("encoding", ["hash", "freq"])
def test_eager_captured_and_one_call_steps_agree_in_default_mode(gpu, encoding):
    """The three paths with the float atomics of default mode, at the bars tests/test_gpu_train_loss.py holds its losses to:
    5e-4 on the loss of every step, 3e-2 on the parameters' norm at the end."""
    torch = gpu
    a, b, c = (_small_trainer(torch, encoding, depth_weight=STEP_LAMBDA) for _ in range(3))
    b.capture_step(900, launch_segments=900 * 30)
    c.entry_args(900, launch_segments=900 * 30)
    for i, (o, d, t, z) in enumerate(_batches(torch, 4)):
        la = float(a.step(o, d, t, z).item())
        Da = a.depth.clone()
        _fill(b, o, d, t, z)
        lb = float(b.step_captured().item())
        Db = b.depth.clone()
        _fill(c, o, d, t, z)
        lc = float(c.step_entry().item())
        assert abs(la - lb) <= 5e-4 * abs(la) and abs(la - lc) <= 5e-4 * abs(la), (i, la, lb, lc)
        for Dx in (Db, c.depth):
            assert float((Da - Dx).abs().max()) <= 5e-4 * float(Da.max()), i
    pa = a.master.cpu().numpy()
    for x in (b, c):
        assert np.linalg.norm(pa - x.master.cpu().numpy()) <= 3e-2 * np.linalg.norm(pa)


def test_inactive_struct_is_the_rung_below_on_gradients_and_step(gpu):
    """rtxn_train_step_depth and rtxn_train_gradients_depth with weight 0 and no outputs against the call without the struct,
    deterministic mode: the same loss, gradients and parameters, bit for bit"""
    torch = gpu
    from rtx_nerf_amd import api
    o, d, t, z = _batches(torch, 1)[0]
    res = []
    for depth in (None, api.train_depth(0.0)):
        tr = _small_trainer(torch, "hash", deterministic=True)
        tr.entry_args(900, launch_segments=900 * 30)
        tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
        tr._det_select()
        api.train_step(tr._entry_args, tr._entry_bg, tr._entry_jit, tr._loss, tr._reg, tr._opt, tr._scaler, tr._ema, depth=depth)
        step_loss, master = tr.loss.clone(), tr.master.clone()
        st = dict(start=tr.start, end=tr.end, seg_view=tr.seg_view, num_stored=tr.num_stored, indices=tr.indices, total=tr.total,
                  targets=tr.graph_targets)
        tr._clear_grads()
        api.train_gradients(tr.net, **tr._batch_kw(st, 900, 900 * 30, None), depth=depth)
        torch.cuda.synchronize()
        res.append((step_loss, master, tr.loss.clone(), tr.dparams.clone(), tr.dtable.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert float(res[0][3].abs().max()) > 0.0


# ---- it supervises ---------------------------------------------------------------------------------------------------------------
# tools/depth_sweep.py's run(): the sphere teacher from 3 training views, 300 steps, hash model, seed 0, deterministic mode, loss
# scale 128; the held-out pose's mean |D - z| over its rays with a target.  Measured on an MI355X (profiles/r25/depth_sweep.txt):
# see E2E_IMPROVEMENT below (held-out PSNR 16.48 -> 17.28 dB beside it); the margin is half of it.
E2E_WEIGHT = 0.1
E2E_IMPROVEMENT = 1.2044e-1 - 8.3616e-2      # the first run on the GPU: 1.2044e-1 without, 8.3616e-2 with depth_weight = 0.1 (316 rays)


def test_depth_supervision_lowers_the_held_out_depth_error(gpu):
    import depth_sweep
    off, on = depth_sweep.run(0.0), depth_sweep.run(E2E_WEIGHT)
    print(f"\ndepth_weight 0: held-out mean |D - z| {off['depth_err']:.4e}, PSNR {off['psnr']:.2f} dB;  depth_weight {E2E_WEIGHT}: "
          f"{on['depth_err']:.4e}, PSNR {on['psnr']:.2f} dB  ({on['rays_with_target']} held-out rays with a target)")
    assert on["rays_with_target"] > 200
    assert on["depth_err"] < off["depth_err"] - 0.5 * E2E_IMPROVEMENT
