"""tests/_ray_gradient_float64.py held to account without a GPU: every GPU test of the ray gradients leans on that restatement, so
its signs, frames and left / right multiplications are checked here against central differences, all in float64.
  * d_origin, d_direction, g_omega, g_tau of a smooth analytic field against (L(+h) - L(-h)) / 2h, L composed through the float64
    make_ray and (R(omega) R0, t0 + tau): h = 1e-4, relative bar 1e-5 (truncation O(h^2) ~ 1e-8, rounding ~ 1e-12);
  * the hash-grid slope against differences of _hashgrid_float64.encode's ref inside a cell, where the interpolant is multilinear
    and the difference quotient along one axis is exact;
  * every seeded defect breaks its derived bound;
  * the kernel's fp32 Rodrigues arithmetic against float64 on both sides of its Taylor threshold, inside the derived bound."""
import numpy as np
import pytest

import _hashgrid_float64 as H
import _ray_gradient_float64 as G

H_STEP, BAR = 1e-4, 1e-5
FOCAL, ASPECT, W, HGT = 1.2, 4.0 / 3.0, 16, 12
FREQ = np.array([[1.3, -0.7, 2.1], [-2.4, 1.9, 0.6], [0.8, 2.7, -1.5]])
PHASE = np.array([0.3, -1.1, 2.0])
AMP = np.array([1.0, 0.6, -0.8])


def field(x):
    return (AMP * np.sin(x @ FREQ.T + PHASE)).sum(axis=-1)


def field_grad(x):
    return (AMP * np.cos(x @ FREQ.T + PHASE)) @ FREQ


def _scene(seed=3, n_images=3, n_rays=7):
    rng = np.random.default_rng(seed)
    poses = []
    for _ in range(n_images):
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        p = np.eye(4)
        p[:3, :3], p[:3, 3] = q, rng.uniform(-3, 3, 3)
        poses.append(p)
    image = rng.integers(0, n_images, n_rays)
    image[:2] = 0, 1                                     # image 2 may stay undrawn on some seeds: count 0 is a case too
    pix = np.stack([rng.integers(0, W, n_rays), rng.integers(0, HGT, n_rays)], 1)
    n_seg = rng.integers(1, 4, n_rays)
    indices = np.concatenate([[0], np.cumsum(n_seg)[:-1]])
    t0 = [np.sort(rng.uniform(0.2, 1.5, 2 * k)) for k in n_seg]
    t_start = np.concatenate([t[0::2] for t in t0])
    t_end = np.concatenate([t[1::2] for t in t0])
    return poses, image, pix, indices, n_seg, t_start, t_end


U_MID = (np.arange(32) + 0.5) / 32


def ray_loss(o, d, ts, te):
    """the restated loss of one ray: the field summed over the 32 midpoint samples of each segment, distances held fixed"""
    total = 0.0
    for a, b in zip(ts, te):
        start, end = o + a * d, o + b * d
        total += field(start[None] + U_MID[:, None] * (end - start)[None]).sum()
    return total


def _analytic(o, d, ts, te):
    """dstart / dend of every segment from the analytic sample gradient, as stage 1 defines them (k = 1)"""
    ds, de = [], []
    for a, b in zip(ts, te):
        start, end = o + a * d, o + b * d
        g = field_grad(start[None] + U_MID[:, None] * (end - start)[None])
        ds.append(((1 - U_MID)[:, None] * g).sum(axis=0))
        de.append((U_MID[:, None] * g).sum(axis=0))
    return np.array(ds), np.array(de)


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_ray_and_pose_gradients_against_central_differences():
    poses, image, pix, indices, n_seg, t_start, t_end = _scene()
    n = len(image)
    rays = [G.make_ray(poses[image[r]], FOCAL, ASPECT, W, HGT, pix[r, 0], pix[r, 1]) for r in range(n)]
    seg = lambda r: slice(indices[r], indices[r] + n_seg[r])
    ds = np.zeros((len(t_start), 3))
    de = np.zeros_like(ds)
    for r, (o, d) in enumerate(rays):
        ds[seg(r)], de[seg(r)] = _analytic(o, d, t_start[seg(r)], t_end[seg(r)])
    do, dd, _, _ = G.ray_reduce(indices, n_seg, t_start, t_end, ds, de)
    fd_o, fd_d = np.zeros((n, 3)), np.zeros((n, 3))
    for r, (o, d) in enumerate(rays):
        for a in range(3):
            e = np.zeros(3)
            e[a] = H_STEP
            ts, te = t_start[seg(r)], t_end[seg(r)]
            fd_o[r, a] = (ray_loss(o + e, d, ts, te) - ray_loss(o - e, d, ts, te)) / (2 * H_STEP)
            fd_d[r, a] = (ray_loss(o, d + e, ts, te) - ray_loss(o, d - e, ts, te)) / (2 * H_STEP)
    assert _rel(do, fd_o) <= BAR and _rel(dd, fd_d) <= BAR, (_rel(do, fd_o), _rel(dd, fd_d))

    grad, _ = G.pose_gradients(image, np.array([d for _, d in rays]), do, dd, len(poses))

    def total_loss(i, delta):
        pose, _ = G.compose_pose(poses[i].ravel(), delta)
        out = 0.0
        for r in np.flatnonzero(image == i):
            o, d = G.make_ray(pose, FOCAL, ASPECT, W, HGT, pix[r, 0], pix[r, 1])
            out += ray_loss(o, d, t_start[seg(r)], t_end[seg(r)])
        return out

    fd = np.zeros((len(poses), 6))
    for i in range(len(poses)):
        for c in range(6):
            e = np.zeros(6)
            e[c] = H_STEP
            fd[i, c] = (total_loss(i, e) - total_loss(i, -e)) / (2 * H_STEP)
        assert grad[i, 6] == (image == i).sum()
    drawn = [i for i in range(len(poses)) if (image == i).any()]
    assert _rel(grad[drawn, :3], fd[drawn, :3]) <= BAR and _rel(grad[drawn, 3:6], fd[drawn, 3:6]) <= BAR
    undrawn = [i for i in range(len(poses)) if i not in drawn]
    assert np.all(grad[undrawn] == 0)


@pytest.mark.parametrize("case", [H.SWEEP[1], H.SWEEP[5], H.SWEEP[7], H.SWEEP[9]], ids=lambda c: "%dx%d-T%d-b%d-s%g" % c)
def test_level_slopes_against_differences_of_the_encoder(case):
    L, F, T, base, s = case
    levels = H.geometry(L, T, base, s)
    table = H.case_table(levels, F, L)
    rng = np.random.default_rng(L + F)
    for l, lv in enumerate(levels):
        if lv.scale == 0:
            continue
        n = 48
        cell = rng.integers(0, max(1, int(lv.scale)), (n, 3))
        fr = rng.uniform(0.3, 0.7, (n, 3))
        x = (2.0 * ((cell + fr - 0.5) / lv.scale) - 1.0).astype(np.float32)
        slope, _, _ = G.level_slopes(levels, F, table, x)
        for a in range(3):
            step = np.float32(0.2 / lv.scale)                       # a tenth of a cell each way: inside the cell
            xp, xm = x.copy(), x.copy()
            xp[:, a] += step
            xm[:, a] -= step
            dx = xp[:, a].astype(np.float64) - xm[:, a].astype(np.float64)
            fd = (H.encode(levels, F, table, xp).ref - H.encode(levels, F, table, xm).ref)[:, l * F:(l + 1) * F] / dx[:, None]
            want = slope[:, l * F:(l + 1) * F, a]
            assert np.abs(fd - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (l, a)


def _gather_case(case, stype):
    L, F, T, base, s = case
    levels = H.geometry(L, T, base, s)
    P = 300
    sp, ep, _ = H.case_segments(levels, 7, P)
    u = G.sample_u(stype, P)
    x = (sp.astype(np.float64).repeat(32, 0) + u[:, None] * (ep.astype(np.float64) - sp.astype(np.float64)).repeat(32, 0)).astype(np.float32)
    table = H.case_table(levels, F, L)
    d, zeroed = H.case_gradient(levels, F, x, L + stype)
    return levels, F, table, x, u, d, zeroed


@pytest.mark.parametrize("defect", G.GATHER_DEFECTS)
def test_gather_defects_break_the_bound(defect):
    broke = []
    for case in H.SWEEP[1:]:                              # the bench grid's float64 arrays are not needed to show a defect
        levels, F, table, x, u, d, zeroed = _gather_case(case, 3)
        assert zeroed <= 0.02
        ds, de, bs, be = G.gather(levels, F, table, x, u, d)
        bs_, be_, _, _ = G.gather(levels, F, table, x, u, d, defect=defect)
        broke.append(bool((np.abs(bs_ - ds) > bs).any() or (np.abs(be_ - de) > be).any()))
        if broke[-1]:
            break
    assert any(broke), defect


def test_near_face_share_of_the_sweep_stays_below_two_percent():
    for case in H.SWEEP[1:]:
        for stype in (0, 3):
            zeroed = _gather_case(case, stype)[-1]
            assert zeroed <= 0.02, (case, stype, zeroed)


def test_ray_and_pose_defects_break_their_bounds():
    rng = np.random.default_rng(11)
    n_seg = np.array([0, 1, 2, 33, 5], np.int32)
    indices = np.concatenate([[0], np.cumsum(n_seg)[:-1]]).astype(np.int32)
    M = int(n_seg.sum())
    ts = np.sort(rng.uniform(0.1, 2.0, (M, 2)), axis=1).astype(np.float32)
    ds, de = rng.standard_normal((M, 3)).astype(np.float32), rng.standard_normal((M, 3)).astype(np.float32)
    do, dd, bo, bd = G.ray_reduce(indices, n_seg, ts[:, 0], ts[:, 1], ds, de)
    _, dd_x, _, _ = G.ray_reduce(indices, n_seg, ts[:, 0], ts[:, 1], ds, de, defect="swap_t")
    assert (np.abs(dd_x - dd) > bd).any()
    assert np.all(do[0] == 0) and np.all(dd[0] == 0) and np.all(bo[0] == 0)
    rays_d = rng.standard_normal((5, 3))
    rays_d = (rays_d / np.linalg.norm(rays_d, axis=1, keepdims=True)).astype(np.float32)
    image = np.array([0, 1, 1, 0, 1])
    grad, bound = G.pose_gradients(image, rays_d, do.astype(np.float32), dd.astype(np.float32), 3)
    for defect in ("cross_order", "tau_no_tenth"):
        bad, _ = G.pose_gradients(image, rays_d, do.astype(np.float32), dd.astype(np.float32), 3, defect=defect)
        assert (np.abs(bad - grad) > bound).any(), defect
    assert np.all(grad[2] == 0)
    pose0 = np.eye(4, dtype=np.float32).ravel()
    delta = np.array([0.3, -0.2, 0.5, 0.0, 0.0, 0.0], np.float32)
    good, b = G.compose_pose(pose0, delta)
    bad, _ = G.compose_pose(pose0, delta, defect="rodrigues_T")
    assert (np.abs(bad - good) > b).any()


@pytest.mark.parametrize("norm", [0.0, 1e-8, 1e-4, 1e-2, 1.0, 3.0, 0.2499, 0.2501])
def test_fp32_rodrigues_matches_float64_on_both_sides_of_the_threshold(norm):
    rng = np.random.default_rng(5)
    for _ in range(8):
        axis = rng.standard_normal(3)
        w = (axis / np.linalg.norm(axis) * norm).astype(np.float32)
        want = G.rodrigues(w)
        assert np.abs(want @ want.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(want) - 1.0) < 1e-14
        got = G.rodrigues_fp32(w).astype(np.float64)
        assert np.all(np.abs(got - want) <= G.rodrigues_bound(w)), (norm, np.abs(got - want).max() / G.rodrigues_bound(w))
    if norm == 0.0:
        assert np.array_equal(G.rodrigues_fp32(np.zeros(3, np.float32)), np.eye(3, dtype=np.float32))
        pose0 = rng.standard_normal(16).astype(np.float32)
        out, b = G.compose_pose(pose0, np.zeros(6, np.float32))
        assert np.array_equal(out.ravel(), pose0.astype(np.float64)) and np.all(b == 0)


def test_one_adam_update_moves_against_the_gradient():
    g = np.array([1e-6, -2e-6, 0.0, 3e-7, 0.0, -1e-9], np.float32)
    d1, m1, v1, t, b_d, b_m, b_v = G.adam_update(np.zeros(6), np.zeros(6), np.zeros(6), 0, g, 1e-3, 0.9, 0.999, 1e-15)
    assert t == 1 and np.all(np.sign(d1) == -np.sign(g))
    assert np.allclose(np.abs(d1[g != 0]), 1e-3, rtol=1e-6)          # the first Adam step is lr sign(g) when eps is below |g|
    assert np.all(b_d >= 0) and np.all(b_m >= 0) and np.all(b_v >= 0)
