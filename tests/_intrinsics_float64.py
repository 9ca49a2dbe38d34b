"""The intrinsics refinement (include/rtxn.h, rtxn_camera_refinement) restated in numpy float64, written from the
header's formulas.  It builds on tests/_camera_float64.py (the models and their converged Newton solves) and on
tests/_ray_gradient_float64.py (adam_update and its derived bounds) by import only and shares no code with the library.
tests/test_intrinsics_float64_reference.py holds it to central differences without a GPU; tests/test_gpu_camera_refine.py holds
the kernels to it.

THE GRADIENT.  ray_terms() returns, per ray, dL/d(fx, fy, cx, cy, k1, k2, k3, k4, p1, p2) for g = dL/dd:
    gw = (g - d (g . d)) / |w|,  gq = R^T gw,  (lx, ly) = dL/d(xd, yd) per model,
    dL/dfx = -lx xd / fx,  dL/dfy = -ly yd / fy,  dL/dcx = -lx / fx,  dL/dcy = -ly / fy
with the lens models differentiated through their solves by the implicit function theorem.  camera_gradients() sums them per
camera and returns the sums beside S = sum_r |term_r| per parameter, the scale every comparison is made on.

THE STEP.  camera_step() is one update of one camera from the fp32 state the kernel started from.  Bounds (U = 2^-24):
  m, v, delta: adam_update's (tests/_ray_gradient_float64.py).  The focal group's gradient is the fp32 product g f, one more
    rounding: U |g f| relative on the gradient, which enters m as (1 - b1) U |g f|, v as 2 (1 - b2) U (g f)^2, and the update
    through both (m's relative error whole, v's halved by the root).
  The clamp is exact.  The row: an additive entry p0 + delta rounds once, U |p|; a focal entry is f0 expf(delta): expf is taken as
    good to 2 ulp (4 U relative; the device library documents 1) and the product rounds once, 5 U |f|.  delta == 0: p0 itself.
"""
import numpy as np

import _camera_float64 as C
from _ray_gradient_float64 import U, adam_update

N_DELTA = 10
NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2")
# the entries a model has: k4 is the fisheye's alone, p1 and p2 the radial-tangential model's
HAS = {C.PINHOLE: (0, 1, 2, 3), C.OPENCV: (0, 1, 2, 3, 4, 5, 6, 8, 9), C.OPENCV_FISHEYE: (0, 1, 2, 3, 4, 5, 6, 7)}
GROUP = (0, 0, 1, 1, 2, 2, 2, 2, 2, 2)          # focal, centre, distortion


def ray_terms(model, p, look_at, px, py, g, scale_k2=1.0):
    """terms [n, 10] in float64 for pixels px, py [n] of the camera row p (float32) under the pose look_at (16 values) and
    g = dL/dd [n, 3].  scale_k2: a seeded defect for the negative control (the k2 term times it)."""
    p64 = np.asarray(p, np.float32).astype(np.float64)
    la = np.asarray(look_at, np.float32).astype(np.float64).reshape(4, 4)
    R = la[:3, :3]
    fx, fy, cx, cy, k1, k2, k3, k4, p1, p2 = p64[:10]
    xd = (np.asarray(px, np.float64) + 0.5 - cx) / fx
    yd = (np.asarray(py, np.float64) + 0.5 - cy) / fy
    q = C.camera_directions(model, p, px, py)
    w = q @ R.T
    nw = np.linalg.norm(w, axis=1, keepdims=True)
    d = w / nw
    g = np.asarray(g, np.float64).reshape(-1, 3)
    gw = (g - d * (g * d).sum(1, keepdims=True)) / nw
    gq = gw @ R
    t = np.zeros((len(xd), N_DELTA))
    lx, ly = gq[:, 0].copy(), gq[:, 1].copy()
    if model == C.OPENCV:
        x, y = q[:, 0], q[:, 1]
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        drad = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2
        j11 = rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
        j22 = rad + 2 * y * y * drad + 2 * p2 * x + 6 * p1 * y
        j12 = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
        det = j11 * j22 - j12 * j12
        lx, ly = (j22 * gq[:, 0] - j12 * gq[:, 1]) / det, (j11 * gq[:, 1] - j12 * gq[:, 0]) / det
        rl = -(lx * x + ly * y)
        t[:, 4], t[:, 5], t[:, 6] = rl * r2, rl * r2 ** 2 * scale_k2, rl * r2 ** 3
        t[:, 8] = -(lx * 2 * x * y + ly * (r2 + 2 * y * y))
        t[:, 9] = -(lx * (r2 + 2 * x * x) + ly * 2 * x * y)
    elif model == C.OPENCV_FISHEYE:
        thd = np.hypot(xd, yd)
        lens = thd >= 1e-8
        safe = np.where(lens, thd, 1.0)
        ux, uy = xd / safe, yd / safe
        th = C.undistort_fisheye(p, thd)
        t2 = th * th
        dpoly = 1 + 3 * k1 * t2 + 5 * k2 * t2 ** 2 + 7 * k3 * t2 ** 3 + 9 * k4 * t2 ** 4
        sn, cs = np.sin(th), np.cos(th)
        gth = cs * (gq[:, 0] * ux + gq[:, 1] * uy) + sn * gq[:, 2]
        a0, a1 = sn * gq[:, 0], sn * gq[:, 1]
        au = a0 * ux + a1 * uy
        gr = gth / dpoly
        lx = np.where(lens, gr * ux + (a0 - au * ux) / safe, lx)
        ly = np.where(lens, gr * uy + (a1 - au * uy) / safe, ly)
        for n in range(1, 5):
            t[:, 3 + n] = np.where(lens, -gr * th ** (2 * n + 1), 0.0) * (scale_k2 if n == 2 else 1.0)
    t[:, 0], t[:, 1] = -lx * xd / fx, -ly * yd / fy
    t[:, 2], t[:, 3] = -lx / fx, -ly / fy
    return t


def camera_gradients(model, params, poses, drawn, width, g, scale_k2=1.0):
    """(grad [n_cameras, 11] = the ten sums and the ray count, S [n_cameras, 10] = sum_r |term_r|) in float64 from fp32 inputs:
    params [n_cameras, 12], poses [n_images, 16], drawn [n, 2] = (image, pixel), g [n, 3].  One camera: every ray is its."""
    params = np.asarray(params, np.float32).reshape(-1, 12)
    drawn = np.asarray(drawn).astype(np.int64).reshape(-1, 2)
    g = np.asarray(g, np.float64).reshape(-1, 3)
    K = params.shape[0]
    grad, S = np.zeros((K, N_DELTA + 1)), np.zeros((K, N_DELTA))
    for c in range(K):
        rows = np.arange(len(drawn)) if K == 1 else np.flatnonzero(drawn[:, 0] == c)
        for i in np.unique(drawn[rows, 0]):
            sel = rows[drawn[rows, 0] == i]
            t = ray_terms(model, params[c], poses[i], drawn[sel, 1] % width, drawn[sel, 1] // width, g[sel], scale_k2)
            grad[c, :N_DELTA] += t.sum(0)
            S[c] += np.abs(t).sum(0)
        grad[c, N_DELTA] = len(rows)
    return grad, S


def compose_row(model, params0, delta):
    """(row [12] float64, bound [12]) from the fp32 row params0 and the fp32 delta [10]"""
    p0 = np.asarray(params0, np.float32).astype(np.float64)
    dl = np.asarray(delta, np.float32).astype(np.float64)
    out, bound = p0.copy(), np.zeros(12)
    for e in HAS[model]:
        if dl[e] == 0:
            continue
        out[e] = p0[e] * np.exp(dl[e]) if e < 2 else p0[e] + dl[e]
        bound[e] = (5 if e < 2 else 1) * U * abs(out[e])
    return out, bound


def camera_step(model, cfg, live, delta, m, v, steps, grad):
    """One update of one camera (count > 0, finite gradient, no skip word) from its fp32 state.  cfg: lr_focal, lr_center,
    lr_distortion, max_log_focal, max_center, max_distortion, beta1, beta2, eps.  live: the camera's live row (the focal gradient is
    dL/df times the live f).  Returns (delta, m, v) float64 [10] with the inactive entries carried over, steps, the bounds
    (b_delta, b_m, b_v) [10] (0 where inactive), and the tuple of active entries; steps is unchanged when none is active."""
    lr = (cfg["lr_focal"], cfg["lr_center"], cfg["lr_distortion"])
    mx = (cfg["max_log_focal"], cfg["max_center"], cfg["max_distortion"])
    live = np.asarray(live, np.float32).astype(np.float64)
    d1, m1, v1 = (np.asarray(a, np.float32).astype(np.float64).copy() for a in (delta, m, v))
    bd, bm, bv = np.zeros(N_DELTA), np.zeros(N_DELTA), np.zeros(N_DELTA)
    active = tuple(e for e in HAS[model] if float(np.float32(lr[GROUP[e]])) > 0)
    if not active:
        return d1, m1, v1, int(steps), bd, bm, bv, active
    t = int(steps)
    o1, o2 = float(np.float32(1.0) - np.float32(cfg["beta1"])), float(np.float32(1.0) - np.float32(cfg["beta2"]))
    for e in active:
        gf = float(np.float32(grad[e]))
        gd = gf * live[e] if e < 2 else gf
        de, me, ve, t, b_d, b_m, b_v = adam_update(d1[e:e + 1], m1[e:e + 1], v1[e:e + 1], steps, np.array([gd]), lr[GROUP[e]],
                                                   cfg["beta1"], cfg["beta2"], cfg["eps"])
        if e < 2:                                  # the fp32 product g f
            upd = abs(float(d1[e] - de[0]))
            b_m = b_m + o1 * U * abs(gd)
            b_v = b_v + 2 * o2 * U * gd * gd
            rel = (o1 * U * abs(gd) / abs(me[0]) if me[0] != 0 else 0.0) + (o2 * U * gd * gd / ve[0] if ve[0] != 0 else 0.0)
            b_d = b_d + upd * rel
        bound = float(np.float32(mx[GROUP[e]]))
        d1[e], m1[e], v1[e] = min(max(de[0], -bound), bound), me[0], ve[0]
        bd[e], bm[e], bv[e] = b_d[0], b_m[0], b_v[0]
    return d1, m1, v1, t, bd, bm, bv, active
