"""Ray gradients and pose refinement (include/rtxn.h) restated in numpy float64, on top of tests/_hashgrid_float64.py,
with DERIVED error bounds per output element.  Nothing here imports the project's kernels or its CPU oracle.
tests/test_ray_gradient_float64_reference.py runs it without a GPU (against central differences and seeded defects),
tests/test_gpu_ray_gradients.py holds the kernels to it.

STAGE 1, the gather.  Sample s = 32 j + i of segment j sits at x = start + u (end - start); per level l (geometry, cell, fractions fr
and corner indices of _hashgrid_float64) the interpolant is multilinear inside the cell, so
    d enc_{l,f} / d x_a = (scale_l / 2) sum_c sgn_a(c) prod_{b != a} w_b(c) T[idx(c)][f]      sgn_a = +1 where bit a of c is set
    g_s[a] = sum_{l, f} d[s][l F + f] d enc_{l,f} / d x_a,   dstart[j][a] = k sum_i (1 - u_i) g_s[a],   dend[j][a] = k sum_i u_i g_s[a]
u is the fp32 value the kernel forms (exact in float64), x the fp32 position the sampler forms.

THE GATHER BOUND (U = 2^-24; per segment, end point and axis), two terms:
  1. arithmetic: c U A.  A = k sum_i weight_i sum_{l,f} |d| (scale_l / 2) sum_c |w_b w_c| |T_c|  -- the absolute values of every
     product that enters the element.  c counts the roundings on the longest path of the order the kernel uses:
       3   a two-factor weight: two subtractions 1 - fr and one product
       8   the corner sum: eight sequential fused multiply-adds (the products themselves are not rounded)
       1   scale / 2 times the sum (the halving itself is exact)
     L F   the level-and-feature sum: one fused multiply-add per (level, feature), sequential
       2   the weight 1 - u (u itself is the kernel's own fp32 value) and its product with g
       5   the butterfly over the half wave's 32 lanes
       1   k
     c = 20 + L F.
  2. position: for a (sample, level) pair FARTHER than tau_l from every face of its cell fp32 and float64 agree on the cell; the slope
     along a is bilinear in the other two fractions, each of which fp32 holds to dfr < (scale_l + 1) 2^-23, and a bilinear form of
     eight corner values moves by at most (max - min) per unit of either fraction taken twice over (both faces of the axis a):
     2 dfr 2 (max - min of the eight corners), times (scale_l / 2) |d|, times the sample's weight and k.
  Pairs NEARER than tau_l: the derivative is discontinuous across the face (the neighbour's slope); case_gradient zeroes d there,
  at most 2 % of a case's pairs (asserted by the callers), so they contribute exactly 0 on both sides.

STAGE 2, per ray:  d_origin[r] = sum_j (dstart_j + dend_j),  d_direction[r] = sum_j (t_start_j dstart_j + t_end_j dend_j).
STAGE 3, per image:  g_omega = sum_r d_r x gd_r,  g_tau = sum_r go_r / 10,  count.
  BOUND of both: (n_terms + c) U sum |terms| -- any order of n_terms additions rounds at most n_terms - 1 times on a path, each
  partial sum at most sum |terms|; c = 2 covers the roundings that are not additions (the fused products are exact, the cross
  product's first product and the division by 10 are one each).

ADAM, one update from the state the kernel started from (the test re-seeds the float64 recurrence from the device's own fp32 state
before every step, so the bound is one step's):  m = b1 m + (1 - b1) g  (1 - b1 is the fp32 value the host forms; one product and one
fused multiply-add: 2 U (|b1 m| + |(1 - b1) g|));  v likewise with g^2 (3 U);  the update lr (m / c1) / (sqrt(v / c2) + eps) carries
m's and half of v's relative error plus: c1 and c2 (1 - b^steps formed in double and rounded once: 1 each, c2 halved by the root), two
divisions, the root, the sum, the product with lr, the last division -- 16 U of |update| covers them with m's 2 and v's 3 / 2 --
and the subtraction from delta rounds once: U |delta'|.

RODRIGUES  R = I + A K + B K^2,  K = [omega]x,  th = |omega|,  A = sin th / th,  B = (1 - cos th) / th^2 = 2 sin^2(th / 2) / th^2.
The kernel uses the series of A and B through th^8 below th = 0.25 (truncation th^10 / 11! < 3e-14) and the closed forms above.
Per element, with w = |omega|:  th^2 is three roundings and the root one (th to 2.5 U relative); sinf is taken as good to 2 ulp
(4 U); A and B are smooth with |th dA/dth|, |th dB/dth| <= 1: err A, err B <= 10 U.  An element is at most three terms
delta_ij, A K_ij, B (omega omega^T - th^2 I)_ij with up to four roundings of their own:
    bound_R = U (10 w + 10 w^2 + 4 (1 + w + w^2 / 2)).
pose = (R R0 | t0 + tau): a three-term dot product, (3 + 1) U sum_k |R_ik R0_kj| + sum_k bound_R |R0_kj|;  the translation U |t0 + tau|.
delta == 0 is poses0 itself, bit for bit.
"""
import numpy as np

import _hashgrid_float64 as H
from _hashgrid_float64 import (SWEEP, _cell, _corners, case_gradient, case_live, case_segments, case_table, geometry,  # noqa: F401
                               near_face)

U = 2.0 ** -24
U32 = np.uint32
GATHER_DEFECTS = ["no_half", "no_scale", "swap_axes", "flip_sign", "swap_u"]
RAY_DEFECTS = ["swap_t"]
POSE_DEFECTS = ["cross_order", "tau_no_tenth", "rodrigues_T"]
TAYLOR = 0.25            # the kernel's threshold on |omega|


# ------------------------------------------------------------------------------------------------ the sample's place in its segment
def fmix32(h):
    h = np.asarray(h, U32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> U32(16)
        h *= U32(0x85EBCA6B)
        h ^= h >> U32(13)
        h *= U32(0xC2B2AE35)
        h ^= h >> U32(16)
    return h


def jitter_offsets(seed, step, n_samples):
    """include/rtxn.h, RTXN_SAMPLING_JITTER_WORLD: float32 [n] in [0, 1), a pure function of (seed, step, s)"""
    with np.errstate(over="ignore"):
        h0 = fmix32((U32(seed) ^ U32(0x5BD1E995)) + U32(0x9E3779B9) * U32(step))
        bits = fmix32(h0 ^ np.arange(n_samples, dtype=U32)) >> U32(8)
    return bits.astype(np.float32) * np.float32(2.0 ** -24)


def sample_u(stype, n_segments, jitter=None):
    """u of every sample, the fp32 value the kernels form, as float64 [32 n].  stype 0: i / 32; 3: (i + 0.5) / 32; 4: (i + jitter_s) / 32
    with jitter = (seed, step)."""
    i = np.tile(np.arange(32, dtype=np.float32), n_segments)
    if stype == 4:
        off = jitter_offsets(jitter[0], jitter[1], 32 * n_segments)
    else:
        off = np.float32(0.5 if stype == 3 else 0.0)
    return ((i + off).astype(np.float32) * np.float32(1.0 / 32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ stage 1
def level_slopes(levels, F, table_f16, x_f32, defect=None):
    """d enc / d x in float64: (slope [n, L F, 3], the sum of absolute products abs [n, L F, 3], the positional allowance pos
    [n, L F, 3] -- per unit of |d|, before the segment weights)."""
    x = np.asarray(x_f32, np.float32)
    n, L = x.shape[0], len(levels)
    total = H.n_entries(levels)
    tab = np.asarray(table_f16, np.float16).astype(np.float64).reshape(-1, F)
    slope, ab, pos = (np.zeros((n, L * F, 3)) for _ in range(3))
    for l, lv in enumerate(levels):
        if lv.scale == 0:
            continue
        g, fr = _cell(lv, x)
        _, idx = _corners(lv, g, fr, total)
        t = tab[idx]                                                        # [n, 8, F]
        hs = lv.scale * (1.0 if defect == "no_half" else 0.5)
        if defect == "no_scale":
            hs = 0.5
        sl = slice(l * F, (l + 1) * F)
        spread = t.max(axis=1) - t.min(axis=1)                              # [n, F]
        for a in range(3):
            w2 = np.ones((n, 8))
            sg = np.ones(8)
            for c in range(8):
                for b in range(3):
                    hi = (c >> b) & 1
                    if b == a:
                        sg[c] = 1.0 if hi else -1.0
                    else:
                        w2[:, c] *= fr[:, b] if hi else 1.0 - fr[:, b]
            if defect == "flip_sign":
                sg = -sg
            out = (a + 1) % 3 if defect == "swap_axes" else a
            slope[:, sl, out] = hs * np.einsum("nc,ncf->nf", w2 * sg, t)
            ab[:, sl, out] = hs * np.einsum("nc,ncf->nf", w2, np.abs(t))
            pos[:, sl, out] = hs * 2.0 * (lv.scale + 1.0) * 2.0 ** -23 * 2.0 * spread
    return slope, ab, pos


def gather(levels, F, table_f16, x_f32, u, denc_f16, k=1.0, defect=None):
    """(dstart, dend, bound_start, bound_end), each [P, 3] float64.  x_f32 [32 P, >= 3] the sampler's positions, u [32 P] from
    sample_u, denc_f16 [32 P, >= L F] sample-major."""
    L = len(levels)
    d = np.asarray(denc_f16, np.float16).astype(np.float64)[:, :L * F]
    slope, ab, pos = level_slopes(levels, F, table_f16, x_f32, defect)
    g = np.einsum("nj,nja->na", d, slope)
    A = np.einsum("nj,nja->na", np.abs(d), ab)
    Pp = np.einsum("nj,nja->na", np.abs(d), pos)
    u = np.asarray(u, np.float64)
    w_end, w_start = (1.0 - u, u) if defect == "swap_u" else (u, 1.0 - u)
    c = 20 + L * F

    def seg(w, v):
        return k * (w[:, None] * v).reshape(-1, 32, 3).sum(axis=1)

    return (seg(w_start, g), seg(w_end, g),
            c * U * seg(w_start, A) + seg(w_start, Pp), c * U * seg(w_end, A) + seg(w_end, Pp))


def check(got, ref, bound):
    """(largest err / bound over the elements with a positive bound, elements NOT inside their bound).  A NaN or an infinity counts;
    an element with bound 0 must be exactly the reference."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    hit = bound > 0
    ratio = float((err[hit] / bound[hit]).max()) if hit.any() else 0.0
    return ratio, int((~(err <= bound)).sum())


# ------------------------------------------------------------------------------------------------ stage 2
def ray_reduce(indices, num_stored, t_start, t_end, dstart, dend, defect=None):
    """(d_origin, d_direction, bound_o, bound_d) [n_rays, 3] float64 from fp32 inputs"""
    ts, te = np.asarray(t_start, np.float64), np.asarray(t_end, np.float64)
    if defect == "swap_t":
        ts, te = te, ts
    ds, de = np.asarray(dstart, np.float64).reshape(-1, 3), np.asarray(dend, np.float64).reshape(-1, 3)
    n = len(indices)
    do, dd, bo, bd = (np.zeros((n, 3)) for _ in range(4))
    for r in range(n):
        j = slice(int(indices[r]), int(indices[r]) + int(num_stored[r]))
        m = 2 * int(num_stored[r])
        do[r] = (ds[j] + de[j]).sum(axis=0)
        dd[r] = (ts[j, None] * ds[j] + te[j, None] * de[j]).sum(axis=0)
        bo[r] = (m + 2) * U * (np.abs(ds[j]) + np.abs(de[j])).sum(axis=0)
        bd[r] = (m + 2) * U * (np.abs(ts[j, None] * ds[j]) + np.abs(te[j, None] * de[j])).sum(axis=0)
    return do, dd, bo, bd


# ------------------------------------------------------------------------------------------------ stage 3
def pose_gradients(drawn_image, rays_d, d_origin, d_direction, n_images, defect=None):
    """(grad [n_images, 7] = g_omega, g_tau, count; bound [n_images, 7]) in float64 from fp32 inputs"""
    d, go, gd = (np.asarray(a, np.float64).reshape(-1, 3) for a in (rays_d, d_origin, d_direction))
    img = np.asarray(drawn_image).astype(np.int64)
    grad, bound = np.zeros((n_images, 7)), np.zeros((n_images, 7))
    for i in range(n_images):
        sel = img == i
        n = int(sel.sum())
        a, b = (gd[sel], d[sel]) if defect == "cross_order" else (d[sel], gd[sel])
        for c in range(3):
            p, q = (c + 1) % 3, (c + 2) % 3
            grad[i, c] = (a[:, p] * b[:, q] - a[:, q] * b[:, p]).sum()
            bound[i, c] = (2 * n + 2) * U * (np.abs(a[:, p] * b[:, q]) + np.abs(a[:, q] * b[:, p])).sum()
        tenth = 1.0 if defect == "tau_no_tenth" else 0.1
        grad[i, 3:6] = tenth * go[sel].sum(axis=0)
        bound[i, 3:6] = (n + 2) * U * 0.1 * np.abs(go[sel]).sum(axis=0)
        grad[i, 6] = n
    return grad, bound


def rodrigues(omega, defect=None):
    """R(omega) in float64: I + A K + B K^2, the series below 1e-4 (where float64's own 1 - cos cancels)"""
    w = np.asarray(omega, np.float64)
    t2 = float(w @ w)
    th = np.sqrt(t2)
    if th < 1e-4:
        A, B = 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    else:
        A, B = np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / t2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    R = np.eye(3) + A * K + B * (K @ K)
    return R.T if defect == "rodrigues_T" else R


def rodrigues_bound(omega):
    w = float(np.linalg.norm(np.asarray(omega, np.float64)))
    return U * (10.0 * w + 10.0 * w * w + 4.0 * (1.0 + w + 0.5 * w * w))


def _f32(x):
    return np.float32(x)


def rodrigues_fp32(omega):
    """The kernel's arithmetic in numpy float32 (a fused multiply-add as a float64 product and sum rounded once): what the CPU test
    holds to rodrigues() on both sides of the threshold."""
    w = np.asarray(omega, np.float32)
    fma = lambda a, b, c: _f32(np.float64(a) * np.float64(b) + np.float64(c))
    t2 = fma(w[2], w[2], fma(w[1], w[1], _f32(w[0] * w[0])))
    th = _f32(np.sqrt(t2))
    if th < _f32(TAYLOR):
        A = fma(t2, fma(t2, fma(t2, fma(t2, _f32(1.0 / 362880), _f32(-1.0 / 5040)), _f32(1.0 / 120)), _f32(-1.0 / 6)), _f32(1.0))
        B = fma(t2, fma(t2, fma(t2, fma(t2, _f32(1.0 / 3628800), _f32(-1.0 / 40320)), _f32(1.0 / 720)), _f32(-1.0 / 24)), _f32(0.5))
    else:
        sh = _f32(np.sin(np.float64(_f32(_f32(0.5) * th))))
        A = _f32(_f32(np.sin(np.float64(th))) / th)
        B = _f32(_f32(_f32(2.0) * _f32(sh * sh)) / t2)
    xx, yy, zz = _f32(w[0] * w[0]), _f32(w[1] * w[1]), _f32(w[2] * w[2])
    xy, xz, yz = _f32(w[0] * w[1]), _f32(w[0] * w[2]), _f32(w[1] * w[2])
    R = np.empty(9, np.float32)
    R[0] = _f32(1.0) - _f32(B * _f32(yy + zz))
    R[4] = _f32(1.0) - _f32(B * _f32(xx + zz))
    R[8] = _f32(1.0) - _f32(B * _f32(xx + yy))
    R[1], R[3] = fma(B, xy, -_f32(A * w[2])), fma(B, xy, _f32(A * w[2]))
    R[2], R[6] = fma(B, xz, _f32(A * w[1])), fma(B, xz, -_f32(A * w[1]))
    R[5], R[7] = fma(B, yz, -_f32(A * w[0])), fma(B, yz, _f32(A * w[0]))
    return R.reshape(3, 3)


def compose_pose(pose0, delta, defect=None):
    """(pose [4, 4] float64, bound [4, 4]) = (R(omega) R0 | t0 + tau ; pose0's last row) from a fp32 pose0 [16] and a fp32 delta [6]"""
    p0 = np.asarray(pose0, np.float64).reshape(4, 4)
    dl = np.asarray(delta, np.float64)
    R = rodrigues(dl[:3], defect)
    out, bound = p0.copy(), np.zeros((4, 4))
    if np.any(dl[:3] != 0):
        out[:3, :3] = R @ p0[:3, :3]
        bound[:3, :3] = rodrigues_bound(dl[:3]) * np.abs(p0[:3, :3]).sum(axis=0)[None, :] + 4 * U * (np.abs(R) @ np.abs(p0[:3, :3]))
    out[:3, 3] = p0[:3, 3] + dl[3:]
    bound[:3, 3] = np.where(dl[3:] != 0, U * np.abs(out[:3, 3]), 0.0)
    return out, bound


def adam_update(delta, m, v, steps, g, lr, beta1, beta2, eps):
    """One update of one image from the fp32 state (delta, m, v [6], steps) and the fp32 gradient g [6]: the new
    (delta, m, v, steps) in float64 and the bounds (b_delta, b_m, b_v) of the module docstring."""
    delta, m, v, g = (np.asarray(a, np.float64) for a in (delta, m, v, g))
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    o1, o2 = float(np.float32(1.0) - np.float32(beta1)), float(np.float32(1.0) - np.float32(beta2))
    lr, eps = float(np.float32(lr)), float(np.float32(eps))
    t = int(steps) + 1
    m1 = b1 * m + o1 * g
    v1 = b2 * v + o2 * g * g
    c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    upd = lr * (m1 / c1) / (np.sqrt(v1 / c2) + eps)
    d1 = delta - upd
    b_m = 2 * U * (np.abs(b1 * m) + np.abs(o1 * g))
    b_v = 3 * U * (np.abs(b2 * v) + np.abs(o2 * g * g))
    b_d = 16 * U * np.abs(upd) + U * np.abs(d1)
    return d1, m1, v1, t, b_d, b_m, b_v


# ------------------------------------------------------------------------------------------------ the camera, for the CPU test
def make_ray(pose, focal, aspect, width, height, px, py):
    """ray_internal.h in float64: the columns of look_at, -focal on the third, the normalisation, the / 10"""
    la = np.asarray(pose, np.float64).reshape(4, 4)
    u = (2 * (px + 0.5) / width - 1) * aspect
    v = 2 * (py + 0.5) / height - 1
    d = la[:3, 0] * u + la[:3, 1] * v - la[:3, 2] * focal
    return la[:3, 3] / 10.0, d / np.linalg.norm(d)
