"""Float64 restatement of the depth term of rtxn_train_depth (include/rtxn.h) and of rtxn_depth_targets' conversion
(a helper module, not a conftest; plain numpy, no torch, no GPU).  Builds on _compositor_float64, whose docstring derives the
bound of the training compositors element by element; this one extends it for the depth addend the way that docstring extends
it for k q_i.  u = 2^-24; no constant comes from running a kernel.

The term, per ray r with the compositor's w_i and the midpoints m_i of the regulariser:
    D = sum_i w_i m_i,  e = D - z,  v = [z finite and > 0],  share = (lambda_z / n_rays) v l(e),  g_D = k_z v l'(e),
    k_z = fl(fl(loss_scale lambda_z) / n_rays)   (fp32, as the host forms it),
    G_i gains g_D m_i,  S gains g_D D.

THE BOUND.  What _compositor_float64 counts, with these additions (a ray with a target; without one g_D = 0 and nothing is added):
  * D as the kernel holds it (Bt, the total of the scans over w m): the scan and the carries are pincl's (k_P additions), m_i is
    three fp32 operations from t_start / t_end and w_i m_i one product (4), and the w's own errors reach it through every sample
    (Ew = sum ew_k, times m_max):
        dD = (k_P + 4) u D + m_max Ew.
  * g_D = fl(k_z l'(fl(D - z))): the subtraction (u |e|) on top of dD, l' with its Lipschitz constant in e (L2: 2, Huber: 1; L1: 0
    away from e = 0, and where |e| <= dD + u |e| the sign itself may differ: 2), the product (u |g_D|):
        dgD = |k_z| Lip (dD + u |e|) + u |g_D|          (L1 at the kink: 2 |k_z|).
  * Gm_i gains |g_D| m_i.  G_i's error gains dgD m_i (D's own error through l') and 5 u |g_D| m_i: m_i's three operations, the
    product and the addition.
  * S gains g_D Bt: its error dgD D + |g_D| dD, and two more operations beside k_S (the product and the addition, each within
    u M with the enlarged Gm).  pincl sums w_i G_i, so G's added error reaches it through every sample: sum_k w_k dG_k.
    fp32(dsigma_i) = d_i [ T_i exp(-x_i) (Gm_i (k_T tmag_i + 12) u + dG_i) + (k_S + k_P + 4) u M + 2 E + E_reg
                           + sum_k w_k (2 dGreg_k + dGdepth_k) + dgD D + |g_D| dD ] + u |ref_i|
  dc_i does not see the term.

rtxn_depth_targets, float64: t = v scale; RAY: t; Z: t / c, c = -(d . l) / |l|, l = pose column 2.  The fp32 expression:
    t = fl(v scale)                                            1 rounding                       (v is exact: uint16, or the float given)
    dot = fl(fl(fl(d0 l0) + fl(d1 l1)) + fl(d2 l2))            within 3 u sum |d_k l_k| (gamma_3, to first order)
    n2 likewise over squares (no cancellation): 3 u n2, halved by the square root (1.5 u), sqrtf correctly rounded (1 u... 0.5 ulp = u)
    c = fl(-dot / norm), target = fl(t / c)                     1 u each
  relative error of the target <= [1 + 3 cond + 1.5 + 1 + 1 + 1] u = (5.5 + 3 cond) u,  cond = sum |d_k l_k| / |d . l| >= 1,
  in units of u = 2^-24, i.e. HALF ulps at worst (a float's ulp is between u and 2 u of its value): TARGET_U(cond) below, with
  the second-order terms covered by a factor (1 + 2^-10).  RAY: 1 u.
"""
from collections import namedtuple

import numpy as np

import _compositor_float64 as c64
from _compositor_float64 import GROW, HALF_SUB16, HALF_ULP16, U, composite_ray, counts, distortion_pairwise, midpoints, ray_slices

F = np.float32
SEGMENTS = (0, 1, 2, 3, 10, 17, 40)        # stored segments per ray: 17 and 40 cross the pair schedule's 512-sample step at K = 32,
KINDS = ("l2", "l1", "huber")              # 10 the one-ray kernel's 64-sample step at K = 7
DELTA = 0.1
LIP = {"l2": 2.0, "l1": 0.0, "huber": 1.0}
N_RAYS = 301


def loss_terms(kind, e, delta=DELTA):
    """float64 l(e), l'(e) of the depth term"""
    if kind == "l2":
        return e * e, 2 * e
    if kind == "l1":
        return np.abs(e), np.sign(e)
    a = np.abs(e)
    return np.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta)), np.clip(e, -delta, delta)


def valid(z):
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0)


_BATCHES = {}


def batch(K):
    """N_RAYS rays, every count of SEGMENTS in turn (shuffled), benign samples thinned to an optical depth of at most 3 per ray;
    made once per K and never changed.  Returns
    (Batch, z float32 [B]): z near the ray's own expected depth (so that e is neither tiny nor huge), about a quarter of the rays
    without a target -- zeros, one negative, one NaN -- and a few exact hits of the Huber kink's either side."""
    if K not in _BATCHES:
        rng = np.random.default_rng(4200 + K)
        segs = [SEGMENTS[i % len(SEGMENTS)] for i in range(N_RAYS)]
        rng.shuffle(segs)
        b = c64._assemble(K, [("benign", int(h)) for h in segs], seed=4300 + K)
        # a long ray of benign samples is opaque after a few dozen of them, and everything behind carries gradients far below fp16's
        # smallest step, where no term can be told from any other: sigma is scaled so that no ray's optical depth exceeds 3
        rad = b.rad.copy()
        for s_ in ray_slices(b):
            tot = float((b.step[s_].astype(np.float64) * rad[s_, 3]).sum())
            if tot > 3.0:
                rad[s_, 3] *= np.float32(3.0 / tot)
        b = b._replace(rad=rad)
        m, _ = midpoints(b)
        z = np.zeros(b.B, np.float32)
        for r, s in enumerate(ray_slices(b)):
            if s.stop > s.start:
                ray = composite_ray(b.rad[s, :3].astype(np.float64), b.rad[s, 3].astype(np.float64), b.step[s].astype(np.float64))
                z[r] = np.float32(float(ray.w @ m[s]) + rng.choice([-1.0, 1.0]) * rng.uniform(0.02, 0.6))
            else:
                z[r] = np.float32(rng.uniform(0.5, 3.0))             # an empty ray with a target: D = 0, e = -z
        z[np.abs(z) < 1e-3] = np.float32(0.5)
        z = np.abs(z)
        none = rng.permutation(b.B)[:b.B // 4]
        z[none] = 0.0
        z[none[0]], z[none[1]] = np.float32(-1.5), np.float32(np.nan)
        _BATCHES[K] = (b, z)
    return _BATCHES[K]


def k_factor(loss_scale, weight, n_rays):
    """k = fl(fl(loss_scale weight) / n_rays): make_depth_args' and make_reg_args' expression, as a float64 value"""
    return float(F(F(loss_scale) * F(weight)) / F(n_rays))


Result = namedtuple("Result", "ref bound pix A L D lz gD dD depth_part")


def gradients(b, z, g, schedule, kind, kz, bg=None, gA=None, reg_k=0.0, delta=DELTA):
    """Float64 radiance gradients [N][4] of the batch with the depth term, and their per-element bound (module docstring), ray by
    ray.  g [B][3], gA [B]: the kernel's own fp16 pixel / alpha gradients as float64; kz = k_factor(...); reg_k: the regulariser's k
    (0: lambda_d = 0 -- the DEPTH kernels still run its arithmetic, with k = 0 exactly, which adds nothing).  Also per ray pixels,
    A, L_r, D, v l(e), g_D, dD, and per element depth_part = the sigma-gradient the depth addend alone contributes."""
    ref, bound, depth_part = np.zeros((b.N, 4)), np.zeros((b.N, 4)), np.zeros(b.N)
    pix, A, L, D, lz, gD, dD = (np.zeros((b.B, 3)), np.zeros(b.B), np.zeros(b.B), np.zeros(b.B), np.zeros(b.B), np.zeros(b.B),
                                np.zeros(b.B))
    m_all, width_all = midpoints(b)
    has = valid(z)
    for r, s in enumerate(ray_slices(b)):
        bgr = np.zeros(3) if bg is None else np.asarray(bg[r], np.float64)
        n = s.stop - s.start
        zr = float(z[r]) if has[r] else 0.0
        if n == 0:
            pix[r] = bgr
            if has[r]:
                l, _ = loss_terms(kind, np.float64(-zr), delta)
                lz[r] = float(l)
            continue
        c, sigma, d = b.rad[s, :3].astype(np.float64), b.rad[s, 3].astype(np.float64), b.step[s].astype(np.float64)
        gr = np.asarray(g[r], np.float64)
        gAr = 0.0 if gA is None else float(gA[r])
        ray = composite_ray(c, sigma, d)
        pix[r], A[r] = ray.col + (1.0 - ray.A) * bgr, ray.A
        kT, kP, kS = counts(schedule, n)
        G = c @ gr - gr @ bgr + gAr
        Gm = np.abs(c) @ np.abs(gr) + np.abs(gr) @ np.abs(bgr) + abs(gAr)
        tmag = ray.tau + ray.x
        if schedule == "pair":
            tmag[0::2] += ray.x[1::2]
        ew = ray.w * (kT * tmag + 4) * U + 2 * U * ray.T * ray.ex * (ray.x != 0)
        Ew = float(ew.sum())
        m, width = m_all[s], width_all[s]
        m_max = float(m.max())
        D[r] = float(ray.w @ m)
        dD[r] = (kP + 4) * U * D[r] + m_max * Ew
        dG_reg, E_reg = 0.0, 0.0
        if reg_k:
            L[r], q = distortion_pairwise(ray.w, m, width)
            Qm = 2 * (m * (3 * ray.A + ray.w) + 3 * m_max * ray.A + ray.w * m) + (2.0 / 3.0) * ray.w * width
            dq = (kP + 9) * U * Qm + 9 * (m + m_max) * Ew
            G = G + reg_k * q
            Gm = Gm + abs(reg_k) * Qm
            dG_reg = abs(reg_k) * dq + 2 * U * abs(reg_k) * Qm
            E_reg = float(ew @ (abs(reg_k) * Qm))
        dG_dep, S_dep = 0.0, 0.0
        if has[r]:
            e = D[r] - zr
            l, dl = loss_terms(kind, np.float64(e), delta)
            lz[r], gD[r] = float(l), kz * float(dl)
            de = dD[r] + U * abs(e)
            lip = LIP[kind]
            if kind == "l1" and abs(e) <= de:
                dgD = 2 * abs(kz)
            else:
                dgD = abs(kz) * lip * de + U * abs(gD[r])
            G = G + gD[r] * m
            Gm = Gm + abs(gD[r]) * m
            dG_dep = dgD * m + 5 * U * abs(gD[r]) * m
            S_dep = dgD * D[r] + abs(gD[r]) * dD[r]
            wGd = ray.w * (gD[r] * m)
            depth_part[s] = d * (ray.T * ray.ex * (gD[r] * m) - (np.cumsum(wGd[::-1])[::-1] - wGd))
        wG = ray.w * G
        suffix = np.cumsum(wG[::-1])[::-1] - wG
        M, E = float(ray.w @ Gm), float(ew @ Gm)
        ref[s, :3] = ray.w[:, None] * gr[None, :]
        ref[s, 3] = d * (ray.T * ray.ex * G - suffix)
        f32_c = np.abs(gr)[None, :] * (ew + U * ray.w)[:, None]
        f32_s = d * (ray.T * ray.ex * (Gm * (kT * tmag + 12) * U + dG_reg + dG_dep) + (kS + kP + 4) * U * M + 2 * E + E_reg
                     + float(np.sum(ray.w * (2 * dG_reg + dG_dep))) + S_dep) + U * np.abs(ref[s, 3])
        bound[s, :3] = HALF_ULP16 * np.abs(ref[s, :3]) * GROW + HALF_SUB16 + GROW * f32_c
        bound[s, 3] = HALF_ULP16 * np.abs(ref[s, 3]) * GROW + HALF_SUB16 + GROW * f32_s
    return Result(ref, bound, pix, A, L, D, lz, gD, dD, depth_part)


def closed_form_sigma_gradient(b, z, g, kind, kz, bg=None, gA=None, reg_k=0.0, delta=DELTA):
    """dL/dsigma [N] by the chain rule through the full Jacobian dw_i/dsigma_j = d_j (T_i exp(-x_i) [i = j] - w_i [j < i]), float64,
    n^2 per ray: no suffix sums, no prefix identities -- what `gradients` must reproduce."""
    out = np.zeros(b.N)
    m_all, width_all = midpoints(b)
    has = valid(z)
    for r, s in enumerate(ray_slices(b)):
        n = s.stop - s.start
        if n == 0:
            continue
        c, sigma, d = b.rad[s, :3].astype(np.float64), b.rad[s, 3].astype(np.float64), b.step[s].astype(np.float64)
        ray = composite_ray(c, sigma, d)
        bgr = np.zeros(3) if bg is None else np.asarray(bg[r], np.float64)
        dLdw = c @ np.asarray(g[r], np.float64) - np.asarray(g[r], np.float64) @ bgr + (0.0 if gA is None else float(gA[r]))
        m = m_all[s]
        if reg_k:
            dLdw = dLdw + reg_k * distortion_pairwise(ray.w, m, width_all[s])[1]
        if has[r]:
            _, dl = loss_terms(kind, np.float64(float(ray.w @ m) - float(z[r])), delta)
            dLdw = dLdw + kz * float(dl) * m
        J = -np.tril(np.repeat(ray.w[:, None], n, 1), -1) + np.diag(ray.T * ray.ex)          # [i][j]
        out[s] = d * (J.T @ dLdw)
    return out


def loss_bar(kind, res, z, delta=DELTA):
    """per ray: how far a kernel's v l(e) may be from the float64 one -- D's error dD and the subtraction's u |e| through the
    slope of l between the two values (L2: 2 (|e| + de); L1: 1; Huber: at most delta), and three roundings of l itself"""
    zz = np.where(valid(z), np.nan_to_num(z.astype(np.float64)), 0.0)
    e = np.abs(res.D - zz)
    de = res.dD + U * e
    slope = {"l2": 2 * (e + de), "l1": np.ones_like(e), "huber": np.full_like(e, delta)}[kind]
    return np.where(valid(z), slope * de + 3 * U * np.abs(res.lz), 0.0)


def moved_share(res, z, b):
    """share of the non-zero sigma-gradients, on rays with a target, that the depth addend alone moves by more than their bound"""
    has = np.repeat(valid(z), b.nh.astype(np.int64) * b.K)
    nz = has & (res.ref[:, 3] != 0.0)
    return float((np.abs(res.depth_part) > res.bound[:, 3])[nz].mean())


# ------------------------------------------------------------------------------------------------------- fp32 restatement
def emulate(b, z, g, schedule, kind, kz, bg=None, gA=None, reg_k=0.0, delta=DELTA):
    """fp32 restatement of composite_train_kernel<true, *, true> ("one") and composite_train_multi_kernel<true, 4, *, true> ("pair")
    over the batch, the pixel gradients g [B][3] and gA [B] given (fp16 values): _compositor_float64.emulate's two sweeps with the
    regulariser always on (k = reg_k, possibly 0) and the depth addend.  Returns (fp16 [N][4], D float32 [B], v l(e) float32 [B])."""
    out = np.full((b.N, 4), np.nan, np.float16)
    Dout, lout = np.zeros(b.B, np.float32), np.zeros(b.B, np.float32)
    lanes = np.arange(64)
    per = 1 if schedule == "one" else 2
    blk = 64 * per
    step_blocks = 1 if schedule == "one" else 4
    rK = F(1.0) / F(b.K)
    kk = np.tile(np.arange(b.K), b.P).astype(np.float32)
    ts_s, te_s = np.repeat(b.ts, b.K), np.repeat(b.te, b.K)
    m_all = ((kk + F(0.5)) * rK) * (te_s - ts_s) + ts_s            # an fma in the kernel: one rounding fewer
    dw_all = (te_s - ts_s) * rK
    kq, kzf, dlt = F(reg_k), F(kz), F(delta)
    scan = c64._scan
    with np.errstate(over="ignore", invalid="ignore"):
        for r, s in enumerate(ray_slices(b)):
            n = s.stop - s.start
            zr = F(z[r])
            has = bool(zr > 0 and np.isfinite(zr))
            if n == 0:
                if has:
                    lout[r] = _loss32(kind, F(0.0) - zr, dlt)[0]
                continue
            npad = -(-n // (blk * step_blocks)) * blk * step_blocks
            c, sig, d = c64._pad(b.rad[s, :3], npad), c64._pad(b.rad[s, 3], npad), c64._pad(b.step[s], npad)
            mm, dwp = c64._pad(m_all[s], npad), c64._pad(dw_all[s], npad)
            g0, g1, g2 = (F(v) for v in g[r])
            bgr = np.zeros(3, np.float32) if bg is None else np.asarray(bg[r], np.float32)
            gAr = F(0.0) if gA is None else F(gA[r])
            gbg = (g0 * bgr[0] + g1 * bgr[1]) + g2 * bgr[2]

            def block(b0, T_carry):
                i = b0 + per * lanes[None, :] + np.arange(per)[:, None]
                cc, ss, dd = c[i], sig[i], d[i]
                x = dd * ss
                if per == 1:
                    incl = scan(x[0])
                    arg = [(T_carry + incl) - x[0]]
                else:
                    pr = x[0] + x[1]
                    incl = scan(pr)
                    T0 = T_carry + (incl - pr)
                    arg = [T0, T0 + x[0]]
                Ti = [np.exp(-a_) for a_ in arg]
                exs = [np.exp(-x[p]) for p in range(per)]
                return i, cc, dd, Ti, exs, incl[63]

            def prefixes(W_carry, M_carry, w, m):
                wm = [w[p] * m[p] for p in range(per)]
                if per == 1:
                    wi, mi = scan(w[0]), scan(wm[0])
                    return [W_carry + (wi - w[0])], [M_carry + (mi - wm[0])], wm, wi[63], mi[63]
                pw, pm = w[0] + w[1], wm[0] + wm[1]
                wi, mi = scan(pw), scan(pm)
                W0, M0 = W_carry + (wi - pw), M_carry + (mi - pm)
                return [W0, W0 + w[0]], [M0, M0 + wm[0]], wm, wi[63], mi[63]

            T_carry = W_carry = M_carry = F(0.0)
            acc = np.zeros((4, 64), np.float32)
            lp, ls = np.zeros(64, np.float32), np.zeros(64, np.float32)
            for b0 in range(0, npad, blk):
                if b0 >= n:
                    break
                i, cc, dd, Ti, exs, tot = block(b0, T_carry)
                w = [Ti[p] * (F(1.0) - exs[p]) for p in range(per)]
                for p in range(per):
                    for ch in range(3):
                        acc[ch] = w[p] * cc[p][:, ch] + acc[ch]
                if per == 1:
                    acc[3] = acc[3] + w[0]
                else:
                    acc[3] = acc[3] + (w[0] + w[1])
                T_carry = T_carry + tot
                Wlt, Mlt, wm, wtot, mtot = prefixes(W_carry, M_carry, w, mm[i])
                for p in range(per):
                    lp = lp + w[p] * (mm[i][p] * Wlt[p] - Mlt[p])
                ls = ls + (w[0] * w[0] if per == 1 else (w[0] * w[0]) + (w[1] * w[1])) * dwp[i][0]
                W_carry, M_carry = W_carry + wtot, M_carry + mtot
            ar, ag, ab, aw = (scan(acc[k])[63] for k in range(4))
            Wt, Bt = W_carry, M_carry
            L = F(2.0) * scan(lp)[63] + scan(ls)[63] * (F(1.0) / F(3.0))
            S = (((g0 * ar + g1 * ag) + g2 * ab) - gbg * aw) + gAr * aw
            S = S + F(2.0) * kq * L
            gD = F(0.0)
            Dout[r] = Bt
            if has:
                lout[r], dl = _loss32(kind, Bt - zr, dlt)
                gD = kzf * dl
            S = S + gD * Bt
            T_carry = P_carry = W_carry = M_carry = F(0.0)
            for b0 in range(0, npad, blk):
                if b0 >= n:
                    break
                i, cc, dd, Ti, exs, tot = block(b0, T_carry)
                a = [F(1.0) - exs[p] for p in range(per)]
                w = [Ti[p] * a[p] for p in range(per)]
                Wlt, Mlt, wm, wtot, mtot = prefixes(W_carry, M_carry, w, mm[i])
                gc = []
                for p in range(per):
                    q = (F(2.0) * (mm[i][p] * ((F(2.0) * Wlt[p] + w[p]) - Wt) - ((F(2.0) * Mlt[p] + wm[p]) - Bt))
                         + (F(2.0) / F(3.0)) * (w[p] * dwp[i][p]))
                    v = ((((g0 * cc[p][:, 0] + g1 * cc[p][:, 1]) + g2 * cc[p][:, 2]) - gbg) + gAr) + kq * q
                    gc.append(v + gD * mm[i][p])
                W_carry, M_carry = W_carry + wtot, M_carry + mtot
                wgc = [w[p] * gc[p] for p in range(per)]
                if per == 1:
                    pincl = [P_carry + scan(wgc[0])]
                    P_next = pincl[0][63]
                else:
                    pin = scan(wgc[0] + wgc[1])
                    pincl1 = P_carry + pin
                    pincl = [pincl1 - wgc[1], pincl1]
                    P_next = P_carry + pin[63]
                for p in range(per):
                    j = b0 + per * lanes + p
                    act = (b0 + per * lanes) < n
                    o = np.stack([g0 * Ti[p] * a[p], g1 * Ti[p] * a[p], g2 * Ti[p] * a[p],
                                  dd[p] * (Ti[p] * exs[p] * gc[p] - (S - pincl[p]))], 1).astype(np.float16)
                    out[s.start + j[act]] = o[act]
                T_carry = T_carry + tot
                P_carry = P_next
    return out, Dout, lout


def _loss32(kind, e, delta):
    """loss_internal.h's loss_term in fp32: (l, l')"""
    e = F(e)
    if kind == "l1":
        return F(abs(e)), F(np.sign(e))
    if kind == "huber":
        a = F(abs(e))
        return (F(0.5) * e * e if a <= delta else delta * (a - F(0.5) * delta)), F(min(max(e, -delta), delta))
    return e * e, F(2.0) * e


# ------------------------------------------------------------------------------------------------------- depth targets
def target_u(cond):
    """the bound of the module docstring on a Z target's relative error, in units of u = 2^-24"""
    return (5.5 + 3.0 * cond) * (1.0 + 2.0 ** -10)


TARGET_U_RAY = 1.0 * (1.0 + 2.0 ** -10)
MIN_COSINE = 2.0 ** -6


def depth_targets(v, scale, kind, rays_d, poses, image):
    """float64 targets [n] and the condition number of each ray's cosine: v the map values of the drawn pixels (any dtype), scale
    the float32 factor the kernel is given, kind "z" | "ray", rays_d [n][3], poses [N][16], image [n].  No target (0): v <= 0 or
    not finite; for "z" also c <= 2^-6."""
    v = np.asarray(v, np.float64)
    t = v * float(F(scale))
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (v > 0)
    d = np.asarray(rays_d, np.float64)
    l = np.asarray(poses, np.float64).reshape(-1, 16)[np.asarray(image)][:, [2, 6, 10]]
    dot = (d * l).sum(1)
    c = -dot / np.sqrt((l * l).sum(1))
    cond = np.abs(d * l).sum(1) / np.maximum(np.abs(dot), 1e-300)
    if kind == "ray":
        return np.where(ok, t, 0.0), np.ones_like(t), c
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok & (c > MIN_COSINE), t / c, 0.0), cond, c
