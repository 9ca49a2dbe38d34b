"""numpy float64 restatement of the camera models of include/rtxn.h (rtxn_camera_set), written from the header's
formulas and sharing no code with the library or with rtx_nerf_amd.api: the forward distortion of the three models, its inverse by
Newton's method run to convergence (50 iterations), and the rays of a whole frame.  The reference of tests/test_gpu_camera.py."""
import numpy as np

PINHOLE, OPENCV, OPENCV_FISHEYE = 0, 1, 2
MODELS = {"pinhole": PINHOLE, "opencv": OPENCV, "opencv_fisheye": OPENCV_FISHEYE}

# (k1, k2, k3, p1, p2): invertible over |x| <= 1, |y| <= 0.75
OPENCV_SETS = [(-0.05, 0.01, 0.0, 0.001, -0.001), (0.12, -0.25, 0.1, 0.002, -0.0015), (-0.3, 0.1, -0.01, 0.001, -0.001),
               (-0.25, 0.07, 0.0, 0.0005, 0.0005)]
# (k1, k2, k3, k4): invertible over theta <= 1.4 rad
FISHEYE_SETS = [(-0.02, 0.003, -0.001, 0.0001), (0.05, -0.01, 0.002, -0.0003), (-0.1, 0.01, 0.0, 0.0)]
# a 40 x 30 frame, off-centre, whose pixels stay inside that field for every set above (test_camera_float64_reference.py checks
# it: the undistorted |x| <= 1, |y| <= 0.75, theta <= 1.4)
W, H, FX, FY, CX, CY = 40, 30, 32.0, 30.0, 18.3, 16.1


def params(fx=FX, fy=FY, cx=CX, cy=CY, k1=0.0, k2=0.0, k3=0.0, k4=0.0, p1=0.0, p2=0.0):
    """one camera row as float32 (what the device reads), twelve values"""
    return np.array([fx, fy, cx, cy, k1, k2, k3, k4, p1, p2, 0.0, 0.0], dtype=np.float32)


def opencv_params(k, **kw):
    return params(k1=k[0], k2=k[1], k3=k[2], p1=k[3], p2=k[4], **kw)


def fisheye_params(k, **kw):
    return params(k1=k[0], k2=k[1], k3=k[2], k4=k[3], **kw)


def all_cases():
    """(name, model, row) of the pinhole and every coefficient set"""
    out = [("pinhole", PINHOLE, params())]
    out += [(f"opencv{i}", OPENCV, opencv_params(k)) for i, k in enumerate(OPENCV_SETS)]
    out += [(f"fisheye{i}", OPENCV_FISHEYE, fisheye_params(k)) for i, k in enumerate(FISHEYE_SETS)]
    return out


def _coeffs(p):
    return tuple(float(v) for v in np.asarray(p, dtype=np.float64)[4:10])


def distort_opencv(p, x, y):
    """undistorted (x, y) -> distorted (xd, yd)"""
    k1, k2, k3, _, p1, p2 = _coeffs(p)
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)


def undistort_opencv(p, xd, yd, iterations=50):
    k1, k2, k3, _, p1, p2 = _coeffs(p)
    x, y = np.array(xd, dtype=np.float64), np.array(yd, dtype=np.float64)
    for _ in range(iterations):
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        drad = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2
        fx, fy = distort_opencv(p, x, y)
        fx, fy = fx - xd, fy - yd
        j11 = rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
        j22 = rad + 2 * y * y * drad + 2 * p2 * x + 6 * p1 * y
        j12 = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
        det = j11 * j22 - j12 * j12
        ok = np.isfinite(det) & (det != 0)
        det = np.where(ok, det, 1.0)
        x = np.where(ok, x - (j22 * fx - j12 * fy) / det, x)
        y = np.where(ok, y - (j11 * fy - j12 * fx) / det, y)
    return x, y


def distort_fisheye(p, theta):
    """undistorted angle -> distorted radius theta_d"""
    k1, k2, k3, k4, _, _ = _coeffs(p)
    t2 = theta * theta
    return theta * (1 + k1 * t2 + k2 * t2 ** 2 + k3 * t2 ** 3 + k4 * t2 ** 4)


def undistort_fisheye(p, theta_d, iterations=50):
    k1, k2, k3, k4, _, _ = _coeffs(p)
    th = np.array(theta_d, dtype=np.float64)
    for _ in range(iterations):
        t2 = th * th
        d = 1 + 3 * k1 * t2 + 5 * k2 * t2 ** 2 + 7 * k3 * t2 ** 3 + 9 * k4 * t2 ** 4
        ok = np.isfinite(d) & (d != 0)
        th = np.where(ok, th - (distort_fisheye(p, th) - theta_d) / np.where(ok, d, 1.0), th)
    return th


def camera_directions(model, p, px, py):
    """camera-space q [n, 3] of pixel indices px, py (arrays) in float64, from the float32 row p"""
    p64 = np.asarray(p, dtype=np.float64)
    xd = (np.asarray(px, dtype=np.float64) + 0.5 - p64[2]) / p64[0]
    yd = (np.asarray(py, dtype=np.float64) + 0.5 - p64[3]) / p64[1]
    if model == PINHOLE:
        return np.stack([xd, yd, -np.ones_like(xd)], -1)
    if model == OPENCV:
        x, y = undistort_opencv(p, xd, yd)
        return np.stack([x, y, -np.ones_like(x)], -1)
    thd = np.hypot(xd, yd)
    th = undistort_fisheye(p, thd)
    small = thd < 1e-8
    s = np.sin(th) / np.where(small, 1.0, thd)
    q = np.stack([s * xd, s * yd, -np.cos(th)], -1)
    q[small] = np.stack([xd, yd, -np.ones_like(xd)], -1)[small]
    return q


def camera_rays(model, p, look_at, width, height):
    """(o, d) float64 [width*height, 3] in launch order (ray = py * width + px) under the float32 pose look_at (16 values)"""
    la = np.asarray(look_at, dtype=np.float32).astype(np.float64).reshape(4, 4)
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    q = camera_directions(model, p, px.reshape(-1), py.reshape(-1))
    d = q @ la[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(la[:3, 3] / 10.0, d.shape).copy()
    return o, d
