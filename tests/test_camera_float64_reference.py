"""The float64 camera reference (tests/_camera_float64.py) against itself and against the project's pinhole helper: what
tests/test_gpu_camera.py measures the device against has to be right first."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _camera_float64 as R  # noqa: E402


def _pose(seed=3):
    """a rotation (QR of a seeded matrix) and a translation, as 16 float32 values"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    la = np.eye(4)
    la[:3, :3], la[:3, 3] = q, rng.uniform(-3, 3, 3)
    return la.astype(np.float32).reshape(16)


def _grid():
    """(xd, yd) of every pixel centre of the test frame, from the float32 row the device reads"""
    p = R.params().astype(np.float64)
    py, px = np.meshgrid(np.arange(R.H), np.arange(R.W), indexing="ij")
    return (px.reshape(-1) + 0.5 - p[2]) / p[0], (py.reshape(-1) + 0.5 - p[3]) / p[1]


@pytest.mark.parametrize("k", R.OPENCV_SETS)
def test_opencv_distort_inverts_undistort(k):
    p = R.opencv_params(k)
    xd, yd = _grid()
    x, y = R.undistort_opencv(p, xd, yd)
    bx, by = R.distort_opencv(p, x, y)
    assert np.abs(bx - xd).max() <= 1e-12 and np.abs(by - yd).max() <= 1e-12
    assert np.abs(x - xd).max() > 1e-4            # the lens does something over this frame
    assert np.abs(x).max() <= 1.0 and np.abs(y).max() <= 0.75      # ... which stays inside the field the set is invertible over


@pytest.mark.parametrize("k", R.FISHEYE_SETS)
def test_fisheye_distort_inverts_undistort(k):
    p = R.fisheye_params(k)
    thd = np.hypot(*_grid())
    th = R.undistort_fisheye(p, thd)
    assert np.abs(R.distort_fisheye(p, th) - thd).max() <= 1e-12
    assert np.abs(th - thd).max() > 1e-4 and th.max() <= 1.4


def test_zero_coefficients_reduce_opencv_to_pinhole_exactly():
    la = _pose()
    o0, d0 = R.camera_rays(R.PINHOLE, R.params(), la, R.W, R.H)
    o1, d1 = R.camera_rays(R.OPENCV, R.params(), la, R.W, R.H)
    assert np.array_equal(d0, d1) and np.array_equal(o0, o1)


def test_zero_coefficient_fisheye_is_the_equidistant_lens():
    """theta = theta_d: the direction makes the angle hypot(xd, yd) with the optical axis"""
    q = R.camera_directions(R.OPENCV_FISHEYE, R.params(), np.arange(R.W), np.full(R.W, 7))
    p = R.params().astype(np.float64)
    xd, yd = (np.arange(R.W) + 0.5 - p[2]) / p[0], (7 + 0.5 - p[3]) / p[1]
    assert np.abs(np.arccos(-q[:, 2] / np.linalg.norm(q, axis=1)) - np.hypot(xd, yd)).max() <= 1e-12


@pytest.mark.parametrize("W,H,focal", [(40, 30, 1.3), (32, 24, 2.7777), (17, 17, 0.9)])
def test_centred_pinhole_is_the_projects_pinhole(W, H, focal):
    """fx = fy = focal H / 2, cx = W / 2, cy = H / 2 is train.camera_rays' camera (aspect W / H): equal within 1e-12.
    train.camera_rays computes in float64 and returns float32, so the comparison is made through that one rounding: the
    returned value must be the float32 nearest to a number within 1e-12 of the reference -- |f32 - ref| <= ulp32(ref) / 2 + 1e-12."""
    import torch  # noqa: F401
    from rtx_nerf_amd import train
    la = _pose(5)
    o32, d32 = train.camera_rays(la, focal, W, H, device="cpu")
    # the parameters in float64 (a float32 row would round focal H / 2)
    p = np.array([focal * H / 2, focal * H / 2, W / 2, H / 2] + [0.0] * 8, dtype=np.float64)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xd, yd = (px.reshape(-1) + 0.5 - p[2]) / p[0], (py.reshape(-1) + 0.5 - p[3]) / p[1]
    la64 = la.astype(np.float64).reshape(4, 4)
    d = np.stack([xd, yd, -np.ones_like(xd)], -1) @ la64[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(la64[:3, 3] / 10.0, d.shape)
    for got, want in ((d32.numpy().astype(np.float64), d), (o32.numpy().astype(np.float64), o)):
        half_ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) / 2
        assert (np.abs(got - want) <= half_ulp + 1e-12).all()
    # and the reference's own frame function is that computation, from a float32 row that holds these values exactly
    if float(np.float32(p[0])) == p[0]:
        _, dr = R.camera_rays(R.PINHOLE, p.astype(np.float32), la, W, H)
        assert np.abs(dr - d).max() <= 1e-12
