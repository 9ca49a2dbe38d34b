"""tests/_intrinsics_float64.py, the float64 restatement of the intrinsics gradient (include/rtxn.h, rtxn_camera_refinement; DESIGN
5.21), held to central finite differences of tests/_camera_float64.py's camera_directions: the eight lens cases, the whole 40 x 30
frame, a pose from scenes.pose_spherical.  No GPU.

L(p) = sum_r g_r . d_r(p), d = normalise(R q(p)).  The step is 1e-6 relative, h = 1e-6 max(|p|, 1): a coefficient that is zero or
1e-4 still gets a step a float64 difference can resolve.  Central differences leave h^2 L''' / 6 (1e-12 relative) of truncation
and about 2^-53 |L| / h (1e-10 relative) of rounding, so 1e-7 of S = sum_r |term_r| per parameter separates a right formula from a
wrong one by three orders of magnitude; the 3 % defect of the negative control is five orders above it."""
import numpy as np
import pytest

import _camera_float64 as CF
import _intrinsics_float64 as I

BOUND = 1e-7


def _pose():
    from rtx_nerf_amd import scenes
    return np.asarray(scenes.pose_spherical(35.0, -25.0, 4.0), np.float32).reshape(16)


def _frame():
    py, px = np.meshgrid(np.arange(CF.H), np.arange(CF.W), indexing="ij")
    return px.reshape(-1), py.reshape(-1)


def _loss(model, p64, la, px, py, g):
    q = CF.camera_directions(model, p64, px, py)
    w = q @ la.astype(np.float64).reshape(4, 4)[:3, :3].T
    return float((g * (w / np.linalg.norm(w, axis=1, keepdims=True))).sum())


def _finite_differences(model, row, la, px, py, g):
    fd = np.zeros(I.N_DELTA)
    for e in range(I.N_DELTA):
        p = row.astype(np.float64)
        h = 1e-6 * max(abs(p[e]), 1.0)
        hi, lo = p.copy(), p.copy()
        hi[e] += h
        lo[e] -= h
        fd[e] = (_loss(model, hi, la, px, py, g) - _loss(model, lo, la, px, py, g)) / (2 * h)
    return fd


def _compare(model, row, scale_k2=1.0):
    la, (px, py) = _pose(), _frame()
    g = np.random.default_rng(21).standard_normal((px.size, 3))
    t = I.ray_terms(model, row, la, px, py, g, scale_k2)
    fd = _finite_differences(model, row, la, px, py, g)
    return t.sum(0), fd, np.abs(t).sum(0)


@pytest.mark.parametrize("name,model,row", CF.all_cases(), ids=[c[0] for c in CF.all_cases()])
def test_the_restated_gradient_agrees_with_central_differences(name, model, row):
    got, fd, S = _compare(model, row)
    ratio = np.abs(got - fd) / np.where(S > 0, S, 1.0)
    print(f"{name}: worst |analytic - central difference| / sum|terms| = {ratio.max():.3g}")
    for e in range(I.N_DELTA):
        if e not in I.HAS[model]:
            assert got[e] == 0.0 and S[e] == 0.0 and fd[e] == 0.0, (name, I.NAMES[e])     # the model does not read the entry
        else:
            assert S[e] > 0 and abs(got[e] - fd[e]) <= BOUND * S[e], (name, I.NAMES[e], ratio[e])


@pytest.mark.parametrize("name,model,row", [c for c in CF.all_cases() if c[1] != CF.PINHOLE], ids=[c[0] for c in CF.all_cases()][1:])
def test_a_k2_term_three_percent_off_fails_the_same_check(name, model, row):
    got, fd, S = _compare(model, row, scale_k2=1.03)
    k2 = I.NAMES.index("k2")
    assert abs(got[k2] - fd[k2]) > BOUND * S[k2], (name, abs(got[k2] - fd[k2]) / S[k2])
    others = [e for e in I.HAS[model] if e != k2]
    assert all(abs(got[e] - fd[e]) <= BOUND * S[e] for e in others)


def test_the_fisheye_principal_point_takes_the_pinhole_form():
    """a pixel centre on the principal point: thd < 1e-8, so fx..cy take the pinhole's gradient and k gets none"""
    row = CF.fisheye_params(CF.FISHEYE_SETS[0], cx=18.5, cy=16.5)
    la = _pose()
    g = np.array([[0.3, -0.7, 0.2]])
    t = I.ray_terms(CF.OPENCV_FISHEYE, row, la, np.array([18]), np.array([16]), g)
    pin = I.ray_terms(CF.PINHOLE, CF.params(cx=18.5, cy=16.5), la, np.array([18]), np.array([16]), g)
    assert np.array_equal(t, pin) and np.all(t[0, 4:] == 0) and np.all(t[0, 2:4] != 0)


def test_compose_and_step_rules():
    cfg = dict(lr_focal=1e-3, lr_center=0.0, lr_distortion=1e-4, max_log_focal=0.5, max_center=4.0, max_distortion=2e-4, beta1=0.9,
               beta2=0.999, eps=1e-15)
    row = CF.opencv_params(CF.OPENCV_SETS[1])
    out, b = I.compose_row(CF.OPENCV, row, np.zeros(10, np.float32))
    assert np.array_equal(out, row.astype(np.float64)) and not b.any()                    # delta == 0: the row itself
    z = np.zeros(10, np.float32)
    grad = np.full(12, 1e-5, np.float32)
    d1, m1, v1, t, bd, bm, bv, active = I.camera_step(CF.OPENCV, cfg, row, z, z, z, 0, grad)
    assert active == (0, 1, 4, 5, 6, 8, 9) and t == 1                                      # the centre is frozen, k4 is not OPENCV's
    assert d1[2] == d1[3] == d1[7] == 0 and bd[2] == bd[7] == 0
    np.testing.assert_allclose(d1[:2], -1e-3, rtol=1e-6)                                   # Adam's first step is its rate
    np.testing.assert_allclose(d1[[4, 5, 6, 8, 9]], -1e-4, rtol=1e-6)
    for _ in range(3):                                                                     # ... and the clamp holds it at the bound
        d1, m1, v1, t, *_ = I.camera_step(CF.OPENCV, cfg, row, d1.astype(np.float32), m1.astype(np.float32), v1.astype(np.float32), t, grad)
    assert np.all(d1[[4, 5, 6, 8, 9]] == -float(np.float32(2e-4))) and t == 4
    out, b = I.compose_row(CF.OPENCV, row, d1.astype(np.float32))
    assert abs(out[0] - float(row[0]) * np.exp(float(np.float32(d1[0])))) == 0 and b[0] > 0 and out[2] == row[2]
