"""Float64 restatement of the TRAINING compositors, per ray and element by element (a helper module, not a conftest; plain numpy,
no torch, no GPU).

The kernels: volrender_bwd_nerf_kernel, volrender_bwd_compat_kernel, volrender_l2_fused_kernel, volrender_l2_fused_multi_kernel<4>,
volrender_l2_bg_kernel, volrender_l2_bg_multi_kernel<4> (rtx_nerf_amd/csrc/volrender.hip) and composite_train_kernel<REG>,
composite_train_multi_kernel<REG, 4> (composite_train.hip).  Two schedules:
    "one"   one sample per lane, 64 per step; the optical depth's prefix T_carry and the prefix P_carry of w (g.c) carried from
            step to step;
    "pair"  two adjacent samples per lane, sub-blocks of 128, four sub-blocks (512 samples) per step; the carries go from
            sub-block to sub-block, the first sample of a pair takes pincl0 = pincl1 - wgc1, and the next step's data is
            prefetched into `nxt` and copied into `cur` at the end of the step.

The quadrature and its exact gradient, as volrender.hip states them, extended as composite_train.hip states it:
    x_i = d_i sigma_i,  tau_i = sum_{k<i} x_k,  T_i = exp(-tau_i),  a_i = 1 - exp(-x_i),  w_i = T_i a_i,
    C = sum w_i c_i,  A = sum w_i,  pixel = C + (1 - A) b,
    dL/dc_i = g w_i,      dL/dsigma_i = d_i (T_i exp(-x_i) G_i - sum_{k>i} w_k G_k),      G_i = g.c_i - g.b + g_A  (+ k q_i, REG).

THE BOUND, per element; u = 2^-24; no constant comes from running a kernel.  Every stored value is one fp32 expression rounded
once to fp16:
    bound = 2^-11 |ref| (1 + 2^-10) + 2^-25 + (1 + 2^-10) fp32      (half an fp16 ulp, taken at the fp32 value; half the fp16
                                                                      subnormal spacing; the fp32 expression's own error)
The fp32 part, counted from the kernels' loops.  steps = ceil(n / 64) (schedule "one"), blocks = ceil(n / 128) ("pair").
  * the exponent of T_i.  "one": fl(fl(T_carry + incl) - x): the product x = d sigma (1), the scan (6 dependent adds), T_carry +
    incl (1), - x (1), and T_carry += lane63(incl) once per earlier step (steps): k_T = 9 + steps.  "pair": the products (1),
    pr = x0 + x1 (1), the scan (6), incl - pr (1), T_carry + (1), T_carry += once per earlier sub-block (blocks), T0 + x0 for
    the second sample (1): k_T = 11 + blocks.  Every partial sum on the way is at most tmag_i = tau_i + x_i, plus the pair's
    second x for a pair's first sample (incl holds it before incl - pr takes it out): |d exponent| <= k_T u tmag_i.
  * the exponential turns that absolute error into a relative one on T_i, and expf is good to 1 ulp (2 u):
    T_i carries (k_T tmag_i + 2) u relative.
  * a_i = 1 - expf(-x_i): the subtraction (u a_i) and expf's ulp as an ABSOLUTE error 2 u exp(-x_i) -- for small x that is far
    more than u a_i.  expf(-0) = 1 exactly: a sample with x = 0 has a = 0 exactly.
    w_i = fl(T a) carries  ew_i = w_i (k_T tmag_i + 4) u + 2 u T_i exp(-x_i) [x_i != 0].
  * dL/dc = fl(fl(g T) a): one more product than w:  |g| (ew_i + u w_i).
  * G_i: three products and two additions on the path (3), - g.b (1), + g_A (1); g.b is itself three roundings of |g|.|b| -- all
    within 5 u Gm_i, Gm_i = |g|.|c_i| + |g|.|b| + |g_A|  (+ the regulariser's part, below).
  * first term T_i exp(-x_i) G_i: T's relative error, expf (2), two products (2), G (5), and the final subtraction's rounding
    charged to it (1):  T_i exp(-x_i) Gm_i (k_T tmag_i + 12) u.
  * the suffix S - pincl_i cancels two sums of the size of M = sum_k w_k Gm_k (over the WHOLE ray):
      pincl: w G formed (w's error apart: one product and G, 6), "one": the scan (6), P_carry + (1), one addition per earlier
             step since P_carry = lane63(pincl) (steps): k_P = 13 + steps.  "pair": wgc0 + wgc1 (1), the scan (6), P_carry + pin
             (1), P_carry += once per earlier sub-block (blocks), pincl0 = pincl1 - wgc1 (1): k_P = 15 + blocks.
      S:     fused kernels: S = g.C - (g.b) A + g_A A from the pixel's sums.  Each sum is a per-lane chain of one fma per sample
             the lane owns ("one": steps; "pair": 2 blocks) and wave_sum (6); then three products and two additions (3),
             (g.b) A and its subtraction (2), g_A A and its addition (2): k_S = steps + 13 | 2 blocks + 13.
             volrender_bwd_nerf_kernel sums w (g.c) per lane (steps) and wave_sum (6), the term formed as above (6): below
             steps + 13 as well.
      the subtraction S - pincl and the last subtraction's rounding charged to the suffix: 2.
      the w's own errors reach S and pincl through every sample each of them sums: at most E = sum_k ew_k Gm_k in either, 2 E in
      all (sweep 2 re-forms the w's of sweep 1 by the same operations, so much of this cancels; the bound does not rely on it).
  * the product with d_i: u |ref|.
    fp32(dsigma_i) = d_i [ T_i exp(-x_i) Gm_i (k_T tmag_i + 12) u + (k_S + k_P + 2) u M + 2 E ] + u |ref_i|
    fp32(dc_i)     = |g| (ew_i + u w_i)
With the regulariser (REG) G_i gains k q_i, q_i = 2 [m_i (2 W_<i + w_i - A) - (2 M_<i + w_i m_i - B)] + (2/3) w_i delta_i.  The
prefixes W_<i and M_<i are scans like pincl's over w and w m (k_P additions), A and B their totals, each at most A or m_max A;
the w's own errors enter every one of them (at most Ew = sum ew_k, times m_max for the w m sums), and the expression itself is
nine more operations:
    Qm_i = 2 [m_i (3 A + w_i) + 3 m_max A + w_i m_i] + (2/3) w_i delta_i       (the expression over absolute values)
    |dq_i| <= (k_P + 9) u Qm_i + 9 (m_i + m_max) Ew          (2 x 4 Ew through the prefixes, the totals and w_i itself, on either
                                                               side; the ninth covers (2/3) delta_i ew_i, delta_i < m_i)
so Gm_i gains |k| Qm_i and G_i's error |k| |dq_i| + 2 u |k| Qm_i (the product and the addition).  S gains 2 k L_r = sum_i w_i (k q_i):
sweep 1 sums it per lane like the colours (within k_S u M with the enlarged Gm), and L_r is quadratic in w, so the w's own errors
reach it twice: E_reg = sum_k ew_k |k| Qm_k once more beside the 2 E.  (m and delta come from t_start / t_end by
three fp32 operations, 3 u m_i: inside the 9.)

The COMPAT backward is the reference project's per-sample formula (not a gradient), with t_{-1} = 0 at the ray's start and no
reset at segment boundaries:  delta = |t_i - t_{i-1}|, tr = delta sigma, e = exp(-sigma delta),
    dc = g tr (1 - e),    dsigma = sum_ch g_ch tr c_ch delta e.
It is held to one fp16 ulp of the float64 value.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
SENTINEL = 0x7E5A                           # an fp16 NaN bit pattern, _train_float64.SENTINEL's (not imported: that module needs the package)
HALF_ULP16 = 2.0 ** -11
HALF_SUB16 = 2.0 ** -25
GROW = 1.0 + 2.0 ** -10
TAIL = 64                                   # half4 records allocated past the last sample
F32_SENTINEL = np.float32(-7.25e30)         # pre-fill of fp32 outputs (pixels, opacity): no kernel result is near it

# ------------------------------------------------------------------------------------------------------- the ladder
# segments per ray, per K.  n = num_hits K samples.
LADDER = {
    32: (0, 1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 48, 128),      # n = 128 one sub-block, 512 one step, 544, 1024, 1056, 4096
    2: (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513),    # one pair either side of every boundary
    1: (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193),
    6: (1, 10, 11, 21, 22, 85, 86),
    7: (1, 9, 10, 18, 19, 73, 74),
    130: (1, 2, 4),
}
REGIMES = ("benign", "dense", "sparse", "impulse", "impulse_before", "transparent")

Batch = namedtuple("Batch", "K B nh idx P N rad step t_regular t_jitter ts te tgt labels starts")


def _regime_samples(rng, regime, n):
    """(sigma, step) of one ray's n samples, float64 values that are exact in float32"""
    if regime == "benign":
        sig, d = rng.uniform(0, 1.5, n), rng.uniform(0, 0.2, n)
    elif regime == "dense":
        sig, d = rng.uniform(0, 40, n), rng.uniform(0.001, 0.06, n)
    elif regime == "sparse":
        sig, d = np.where(rng.uniform(0, 1, n) < 0.05, rng.uniform(5, 80, n), 0.0), rng.uniform(0.001, 0.06, n)
    elif regime in ("impulse", "impulse_before"):
        sig, d = np.zeros(n), rng.uniform(0.01, 0.2, n)
        j = (n - 1) // 64 * 64 - (1 if regime == "impulse_before" else 0)
        sig[j] = rng.uniform(1, 5) / d[j]
    else:
        sig, d = np.zeros(n), rng.uniform(0, 0.2, n)
        d[::3] = 0.0
    return sig.astype(np.float32), d.astype(np.float32)


def _assemble(K, rays, seed):
    """rays: list of (regime, num_hits) in the order they are laid out"""
    rng = np.random.default_rng(seed)
    B = len(rays)
    nh = np.array([h for _, h in rays], np.int32)
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)          # the exclusive scan include/rtxn.h requires
    P = int(nh.sum())
    N = P * K
    starts = np.concatenate([[0], np.cumsum(nh.astype(np.int64) * K)])
    rad = np.zeros((N, 4), np.float32)
    step = np.zeros(N, np.float32)
    rad[:, :3] = rng.uniform(0, 1, (N, 3))
    for r, (regime, h) in enumerate(rays):
        if h:
            s = slice(int(starts[r]), int(starts[r + 1]))
            rad[s, 3], step[s] = _regime_samples(rng, regime, h * K)
    k = np.tile(np.arange(K), P)
    t_regular = ((k + 1).astype(np.float32) * (np.float32(1.0) / np.float32(K))).astype(np.float32)     # sampler's REGULAR t_vals
    t_jitter = ((k + rng.uniform(0, 1, N)) / K).astype(np.float32)
    # ascending disjoint segments per ray for the regulariser: every second gap 0, the step lengths are NOT tied to them (the
    # compositor reads the distances from t_start / t_end only)
    ts, te = np.zeros(P, np.float32), np.zeros(P, np.float32)
    length = (rng.uniform(0.01, 0.2, P) * min(K, 32)).astype(np.float32)
    gap = (rng.uniform(0.0, 0.3, P) * rng.integers(0, 2, P)).astype(np.float32)
    first = rng.uniform(0.1, 1.0, B).astype(np.float32)
    for r in range(B):
        t = first[r]
        for j in range(idx[r], idx[r] + nh[r]):
            ts[j] = t
            te[j] = np.float32(t + length[j])
            t = np.float32(te[j] + gap[j])
    tgt = rng.uniform(0, 1, (B, 4)).astype(np.float32)
    tgt[::5, 3] = 0.0
    tgt[1::5, 3] = 1.0
    return Batch(K, B, nh, idx, P, N, rad, step, t_regular, t_jitter, ts, te, tgt, list(rays), starts)


_BATCHES = {}


def ladder(K):
    """Every length of LADDER[K] once per regime in ONE batch, laid out in a fixed shuffled order (a 4096-sample ray shares its
    block of four with empty and short ones).  impulse_before needs a sample before the last multiple of 64: rays shorter than
    65 samples have none and are left out of that regime.  Made once, never changed."""
    if ("ladder", K) not in _BATCHES:
        rays = [(regime, h) for regime in REGIMES for h in LADDER[K]
                if not (regime == "impulse_before" and (h * K - 1) // 64 == 0) and not (h == 0 and regime != "benign")]
        rays += [("benign", 0)] * 3 if K == 32 else [("benign", 0)]           # empty rays among the long ones
        order = np.random.default_rng(1000 + K).permutation(len(rays))
        _BATCHES[("ladder", K)] = _assemble(K, [rays[i] for i in order], seed=2000 + K)
    return _BATCHES[("ladder", K)]


def small(B):
    """B = 1 and B = 5 from the K = 32 ladder: the last (only) block of four waves has idle waves while the loss is reduced"""
    rays = {1: [("impulse_before", 33)], 5: [("dense", 128), ("benign", 0), ("impulse_before", 33), ("transparent", 17), ("sparse", 32)]}[B]
    if ("small", B) not in _BATCHES:
        _BATCHES[("small", B)] = _assemble(32, rays, seed=3000 + B)
    return _BATCHES[("small", B)]


def old_shapes(K, B=777, seed=1026):
    """A batch drawn the way the existing tests draw theirs, with num_hits <= 12 (tests/test_gpu_train.py, test_golden.py: no ray
    above 384 samples at K = 32): benign samples only."""
    if ("old", K, B, seed) not in _BATCHES:
        rng = np.random.default_rng(seed + K)
        nh = rng.integers(0, 13, B)
        nh[::7] = 0
        _BATCHES[("old", K, B, seed)] = _assemble(K, [("benign", int(h)) for h in nh], seed=seed + 7 * K)
    return _BATCHES[("old", K, B, seed)]


def as_batch(K, nh, rad, step, tgt, regime="benign"):
    """a batch some other test made (num_hits, radiance, step lengths, targets) in this module's form; no t_vals, no segments"""
    nh = np.asarray(nh, np.int32)
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
    P = int(nh.sum())
    starts = np.concatenate([[0], np.cumsum(nh.astype(np.int64) * K)])
    return Batch(K, nh.size, nh, idx, P, P * K, rad, step, None, None, None, None, tgt, [(regime, int(h)) for h in nh], starts)


def ray_slices(b):
    return [slice(int(b.starts[r]), int(b.starts[r + 1])) for r in range(b.B)]


def label(b, r):
    regime, h = b.labels[r]
    return f"{regime} n={h * b.K}"


# ------------------------------------------------------------------------------------------------------- the loss table
def composited_target(bg, tgt):
    """the target the kernel fits: RGBA composited over the background in fp32 (include/rtxn.h); float64 out"""
    if tgt.shape[1] == 3:
        return tgt.astype(np.float64)
    a = tgt[:, 3:4]
    t = a * tgt[:, :3] + (np.float32(1.0) - a) * np.asarray(bg, np.float32)
    assert t.dtype == np.float32
    return t.astype(np.float64)


def loss_terms(kind, e, p, param):
    """float64 l(e) and dl/dp of include/rtxn.h's table; param: Huber's delta, relative L2's epsilon"""
    if kind == "l2":
        return e * e, 2 * e
    if kind == "l1":
        return np.abs(e), np.sign(e)
    if kind == "huber":
        a = np.abs(e)
        return np.where(a <= param, 0.5 * e * e, param * (a - 0.5 * param)), np.clip(e, -param, param)
    den = p * p + param
    return e * e / den, 2 * e / den


LIPSCHITZ = {"l2": 2.0, "huber": 1.0}        # of dl/dp in the pixel


def half_order(x):
    """fp16 values as integers ordered like the values: differences are distances in units of the last place"""
    i = np.ascontiguousarray(x).view(np.int16).astype(np.int32)
    return np.where(i < 0, -(i & 0x7FFF), i)


def check_loss_gradients(got, want64, slack):
    """got: the kernel's fp16 loss gradients; want64: LS dl / (3 B) in float64; slack: how far the kernel's fp32 value may be
    from want64 (the pixel bar through dl/dp, plus the fp32 roundings).  Every element within one ulp of half(want64); one that
    differs lies within `slack` of the rounding boundary between the two fp16 values.  Returns (differing, max ulps)."""
    with np.errstate(over="ignore"):
        h = want64.astype(np.float16)
    ulps = np.abs(half_order(got) - half_order(h))
    assert ulps.max() <= 1, f"fp16 loss gradients up to {int(ulps.max())} ulp from half(float64)"
    differ = ulps != 0
    mid = (got.astype(np.float64) + h.astype(np.float64)) / 2          # the boundary between the two neighbouring fp16 values
    off = np.abs(want64 - mid)
    bad = differ & (off > slack)
    assert not bad.any(), (f"{int(bad.sum())} fp16 loss gradients differ from half(float64) although float64 lies up to "
                           f"{(off / np.maximum(slack, 1e-300))[bad].max():.2f} slacks from the rounding boundary")
    return int(differ.sum()), int(ulps.max())


# ------------------------------------------------------------------------------------------------------- the reference
Ray = namedtuple("Ray", "x tau T ex a w col A")


def composite_ray(c, sigma, d):
    """float64 forward of one ray: c [n][3], sigma [n], d [n]"""
    x = d * sigma
    tau = np.cumsum(x) - x
    T, ex = np.exp(-tau), np.exp(-x)
    a = -np.expm1(-x)
    w = T * a
    return Ray(x, tau, T, ex, a, w, w @ c, float(w.sum()))


def distortion_pairwise(w, m, width):
    """float64 of one ray: L_r = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i (the PAIRWISE double sum include/rtxn.h
    defines) and q = dL_r/dw = 2 sum_j w_j |m_i - m_j| + (2/3) w_i delta_i, in rows of at most 512 to bound the memory."""
    n = w.shape[0]
    q = np.zeros(n)
    L = 0.0
    for i0 in range(0, n, 512):
        D = np.abs(m[i0:i0 + 512, None] - m[None, :])
        row = D @ w
        L += float(w[i0:i0 + 512] @ row)
        q[i0:i0 + 512] = 2.0 * row
    return L + float((w * w * width).sum()) / 3.0, q + (2.0 / 3.0) * w * width


def midpoints(b):
    """float64 per sample: midpoint m and width delta of its sub-interval, from the segments' t_start / t_end"""
    k = np.tile(np.arange(b.K, dtype=np.float64), b.P)
    ts, te = np.repeat(b.ts.astype(np.float64), b.K), np.repeat(b.te.astype(np.float64), b.K)
    return ts + (k + 0.5) / b.K * (te - ts), (te - ts) / b.K


def counts(schedule, n):
    """(k_T, k_P, k_S) of the module docstring"""
    if schedule == "one":
        steps = -(-n // 64)
        return 9 + steps, 13 + steps, steps + 13
    blocks = -(-n // 128)
    return 11 + blocks, 15 + blocks, 2 * blocks + 13


Gradients = namedtuple("Gradients", "ref bound mag pix A L depth")


def gradients(b, g, schedule, bg=None, gA=None, reg_k=0.0):
    """Float64 radiance gradients [N][4] of the whole batch and their per-element bound, ray by ray.
    g [B][3]: the pixel gradients the kernel used (its own fp16 values, as float64); bg [B][3] or None; gA [B] or None (the alpha
    term's fp16 gradient); reg_k: the factor k of q_i (0: no regulariser).  Also mag [N][4], the sizes the fp32 part scales with (|g| T_i;
    d_i (T_i exp(-x_i) Gm_i + M)), pixels [B][3], A [B], L_r [B], sum w m [B]."""
    ref, bound, mag = np.zeros((b.N, 4)), np.zeros((b.N, 4)), np.zeros((b.N, 4))
    pix, A, L, depth = np.zeros((b.B, 3)), np.zeros(b.B), np.zeros(b.B), np.zeros(b.B)
    if reg_k:
        m_all, width_all = midpoints(b)
    for r, s in enumerate(ray_slices(b)):
        bgr = np.zeros(3) if bg is None else np.asarray(bg[r], np.float64)
        n = s.stop - s.start
        if n == 0:
            pix[r] = bgr
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
        dG_reg, E_reg = 0.0, 0.0
        if reg_k:
            m, width = m_all[s], width_all[s]
            L[r], q = distortion_pairwise(ray.w, m, width)
            depth[r] = float(ray.w @ m)
            m_max = float(m.max())
            Qm = 2 * (m * (3 * ray.A + ray.w) + 3 * m_max * ray.A + ray.w * m) + (2.0 / 3.0) * ray.w * width
            dq = (kP + 9) * U * Qm + 9 * (m + m_max) * float(ew.sum())
            G = G + reg_k * q
            Gm = Gm + abs(reg_k) * Qm
            dG_reg = abs(reg_k) * dq + 2 * U * abs(reg_k) * Qm
            E_reg = float(ew @ (abs(reg_k) * Qm))
        wG = ray.w * G
        suffix = np.cumsum(wG[::-1])[::-1] - wG
        M, E = float(ray.w @ Gm), float(ew @ Gm)
        ref[s, :3] = ray.w[:, None] * gr[None, :]
        ref[s, 3] = d * (ray.T * ray.ex * G - suffix)
        f32_c = np.abs(gr)[None, :] * (ew + U * ray.w)[:, None]
        # the regulariser's part of G's error (dG_reg) reaches the first term directly and S and pincl through every sample they sum
        f32_s = d * (ray.T * ray.ex * (Gm * (kT * tmag + 12) * U + dG_reg) + (kS + kP + 2) * U * M + 2 * E + E_reg
                     + 2 * float(np.sum(ray.w * dG_reg))) + U * np.abs(ref[s, 3])
        mag[s, :3] = np.abs(gr)[None, :] * ray.T[:, None]
        mag[s, 3] = d * (ray.T * ray.ex * Gm + M)
        bound[s, :3] = HALF_ULP16 * np.abs(ref[s, :3]) * GROW + HALF_SUB16 + GROW * f32_c
        bound[s, 3] = HALF_ULP16 * np.abs(ref[s, 3]) * GROW + HALF_SUB16 + GROW * f32_s
    return Gradients(ref, bound, mag, pix, A, L, depth)


def compat_backward(b, g, t_vals):
    """float64 [N][4] of the COMPAT per-sample formula; t_{-1} = 0 per ray, not reset at segment boundaries"""
    out = np.zeros((b.N, 4))
    for r, s in enumerate(ray_slices(b)):
        if s.stop == s.start:
            continue
        c, sigma, t = b.rad[s, :3].astype(np.float64), b.rad[s, 3].astype(np.float64), t_vals[s].astype(np.float64)
        delta = np.abs(t - np.concatenate([[0.0], t[:-1]]))
        tr, e = delta * sigma, np.exp(-sigma * delta)
        gr = np.asarray(g[r], np.float64)
        out[s, :3] = gr[None, :] * (tr * -np.expm1(-sigma * delta))[:, None]
        out[s, 3] = (gr[None, :] * tr[:, None] * c * (delta * e)[:, None]).sum(1)
    return out


# ------------------------------------------------------------------------------------------------------- the shared assertions
def check_elements(what, got, ref, bound, b=None):
    """THE assertion: every element of `got` (fp16 [N][4]) is finite and within `bound` of `ref`; none is left out.  Returns per
    regime (largest err / bound, share of elements above half the bound, largest fp32 error SHOWN / fp32 part of the bound) when
    the batch is given.  The third figure: a stored value that is not half(ref) proves that the kernel's fp32 value lay on the
    other side of the rounding boundary between the two, i.e. at least |ref - boundary| from ref; a stored value that is
    half(ref) proves nothing and counts 0.  A largest err / bound near 1 beside a small third figure is the fp16 term, which
    lands at 1.0 by construction; a third figure near 1 would call for a recount of k."""
    got = np.asarray(got)
    assert got.dtype == np.float16 and got.shape == ref.shape == bound.shape, (what, got.dtype, got.shape, ref.shape)
    v = got.astype(np.float64)
    finite = np.isfinite(v)
    ratio = np.where(finite, np.abs(v - ref), np.inf) / bound
    with np.errstate(over="ignore"):
        nearest = ref.astype(np.float16).astype(np.float64)            # half(ref): what exact arithmetic would have stored
    fp32_part = (bound - HALF_SUB16 - HALF_ULP16 * np.abs(ref) * GROW) / GROW
    shown = np.where(finite & (v != nearest), np.abs(ref - (v + nearest) / 2), 0.0) / np.maximum(fp32_part, 1e-300)
    table = {}
    if b is not None:
        for regime in REGIMES:
            rows = [s for s, (rg, _) in zip(ray_slices(b), b.labels) if rg == regime and s.stop > s.start]
            if rows:
                x = np.concatenate([ratio[s].reshape(-1) for s in rows])
                table[regime] = (float(x.max()), float((x > 0.5).mean()), max(float(shown[s].max()) for s in rows))
    bad = ratio > 1.0
    if bad.any():
        where = ""
        if b is not None:
            hit = sorted({label(b, r) for r, s in enumerate(ray_slices(b)) if bad[s].any()})
            where = f"; rays: {', '.join(hit[:12])}{' ...' if len(hit) > 12 else ''}"
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound ({int((~finite).sum())} not finite), "
                             f"largest err / bound {ratio[i]:.3g} at {i} (got {v[i]:.6g}, ref {ref[i]:.6g}){where}")
    return table


def failing_rays(got, ref, bound, b):
    """labels of the rays with an element outside the bound (or not finite)"""
    v = np.asarray(got).astype(np.float64)
    bad = ~(np.abs(v - ref) <= bound)
    return sorted({label(b, r) for r, s in enumerate(ray_slices(b)) if bad[s].any()})


def table_lines(title, table):
    return [f"measured {title} {regime}: err / bound {m:.3f}, above half the bound {h:.4f}, fp32 error shown / fp32 part {f:.3f}"
            for regime, (m, h, f) in table.items()]


def is_sentinel(a):
    return np.ascontiguousarray(a).view(np.uint16) == SENTINEL


def check_written(got_with_tail, N):
    """got_with_tail: fp16 [N + TAIL][4] pre-filled with SENTINEL: the tail is untouched, every in-range element written"""
    assert got_with_tail.shape[0] >= N + TAIL
    assert is_sentinel(got_with_tail[N:]).all(), "the tail past the last sample was written"
    left = is_sentinel(got_with_tail[:N])
    assert not left.any(), f"{int(left.sum())} in-range gradient elements were never written, first at {np.argwhere(left)[0]}"


# ------------------------------------------------------------------------------------------------------- fp32 restatements
def _scan(v):
    """inclusive scan over the 64 lanes in six dependent fp32 additions (wave_incl_scan_f's depth)"""
    v = v.astype(np.float32).copy()
    for s in (1, 2, 4, 8, 16, 32):
        v[s:] = v[s:] + v[:-s]
    return v


F = np.float32
DEFECTS_PAIR = ("P_carry_step", "P_carry_block", "T_carry_step", "pincl0_is_pincl1", "inclusive_T", "stale_cur", "short_mask", "S_without_bg")
DEFECTS_ONE = ("P_carry_step", "T_carry_step", "inclusive_T", "short_mask", "S_without_bg")


def _pad(a, n):
    out = np.zeros((n,) + a.shape[1:], np.float32)
    out[:a.shape[0]] = a
    return out


def emulate(b, g, schedule, bg=None, gA=None, defect=None, S_from="pixel", reg_k=0.0):
    """fp32 restatement of sweep 1 and sweep 2 of a schedule over the batch, the pixel gradients g [B][3] given (fp16 values);
    fp16 [N][4] out, NaN where nothing was stored.  S_from: "pixel" (the fused kernels: g.C - (g.b) A + g_A A) or "sum"
    (volrender_bwd_nerf_kernel: sum of w (g.c)).  defect: one of DEFECTS_*, planted; None: faithful.  reg_k: the regulariser's factor
    k of q_i (composite_train_*<true>), the midpoints and widths from the batch's t_start / t_end."""
    out = np.full((b.N, 4), np.nan, np.float16)
    lanes = np.arange(64)
    per = 1 if schedule == "one" else 2
    blk = 64 * per
    blocks_per_step = 1 if schedule == "one" else 4
    if reg_k:
        rK = F(1.0) / F(b.K)
        kk = np.tile(np.arange(b.K), b.P).astype(np.float32)
        ts_s, te_s = np.repeat(b.ts, b.K), np.repeat(b.te, b.K)
        m_all = ((kk + F(0.5)) * rK) * (te_s - ts_s) + ts_s          # an fma in the kernel
        dw_all = (te_s - ts_s) * rK
        kq = F(reg_k)
    with np.errstate(over="ignore", invalid="ignore"):
        for r, s in enumerate(ray_slices(b)):
            n = s.stop - s.start
            if n == 0:
                continue
            npad = -(-n // (blk * blocks_per_step)) * blk * blocks_per_step
            c, sig, d = _pad(b.rad[s, :3], npad), _pad(b.rad[s, 3], npad), _pad(b.step[s], npad)
            if reg_k:
                mm, dwp = _pad(m_all[s], npad), _pad(dw_all[s], npad)
            g0, g1, g2 = (F(v) for v in g[r])
            bgr = np.zeros(3, np.float32) if bg is None else np.asarray(bg[r], np.float32)
            gAr = F(0.0) if gA is None else F(gA[r])
            gbg = (g0 * bgr[0] + g1 * bgr[1]) + g2 * bgr[2]

            def data(b0, step0):
                """the block's samples as the kernel holds them: [per][64]; stale_cur: the first step's registers again"""
                src = b0 - step0 if defect == "stale_cur" else b0
                i = src + per * lanes[None, :] + np.arange(per)[:, None]
                return c[i], sig[i], d[i]

            def prefixes(W_carry, M_carry, w, m):
                """REG: W_<i and M_<i of the block's samples [per][64], and the block's totals"""
                wm = [w[p] * m[p] for p in range(per)]
                if per == 1:
                    wi, mi = _scan(w[0]), _scan(wm[0])
                    return [W_carry + (wi - w[0])], [M_carry + (mi - wm[0])], wm, wi[63], mi[63]
                pw, pm = w[0] + w[1], wm[0] + wm[1]
                wi, mi = _scan(pw), _scan(pm)
                W0, M0 = W_carry + (wi - pw), M_carry + (mi - pm)
                return [W0, W0 + w[0]], [M0, M0 + wm[0]], wm, wi[63], mi[63]

            def weights(T_carry, cc, ss, dd):
                x = dd * ss
                if per == 1:
                    incl = _scan(x[0])
                    arg = [(T_carry + incl) - x[0]]
                    if defect == "inclusive_T":
                        arg = [T_carry + incl]
                    tot = incl[63]
                else:
                    pr = x[0] + x[1]
                    incl = _scan(pr)
                    T0 = T_carry + (incl - pr)
                    arg = [T0, T0 + x[0]]
                    if defect == "inclusive_T":
                        arg = [T0 + x[0], (T0 + x[0]) + x[1]]
                    tot = incl[63]
                Ti = [np.exp(-a_) for a_ in arg]
                exs = [np.exp(-x[p]) for p in range(per)]
                return x, Ti, exs, tot

            # sweep 1
            T_carry = F(0.0)
            acc = np.zeros((4, 64), np.float32)                   # r, g, b, w per lane
            Ssum = np.zeros(64, np.float32)
            W_carry = M_carry = F(0.0)
            lp, ls = np.zeros(64, np.float32), np.zeros(64, np.float32)
            for b0 in range(0, npad, blk):
                step0 = b0 // (blk * blocks_per_step) * (blk * blocks_per_step)
                if b0 >= n:
                    break
                if defect == "T_carry_step" and b0 == step0 and b0 > 0:
                    T_carry = F(0.0)
                cc, ss, dd = data(b0, step0)
                x, Ti, exs, tot = weights(T_carry, cc, ss, dd)
                for p in range(per):
                    w = Ti[p] * (F(1.0) - exs[p])
                    for ch in range(3):
                        acc[ch] = w * cc[p][:, ch] + acc[ch]          # an fma in the kernel: one rounding fewer
                    acc[3] = acc[3] + w
                    Ssum = Ssum + w * ((g0 * cc[p][:, 0] + g1 * cc[p][:, 1]) + g2 * cc[p][:, 2])
                T_carry = T_carry + tot
                if reg_k:
                    i = b0 + per * lanes[None, :] + np.arange(per)[:, None]
                    w = [Ti[p] * (F(1.0) - exs[p]) for p in range(per)]
                    Wlt, Mlt, wm, wtot, mtot = prefixes(W_carry, M_carry, w, mm[i])
                    for p in range(per):
                        lp = lp + w[p] * (mm[i][p] * Wlt[p] - Mlt[p])
                    ls = ls + (w[0] * w[0] if per == 1 else (w[0] * w[0]) + (w[1] * w[1])) * dwp[i][0]
                    W_carry, M_carry = W_carry + wtot, M_carry + mtot
            ar, ag, ab, aw = (_scan(acc[k])[63] for k in range(4))
            if S_from == "sum":
                S = _scan(Ssum)[63]
            else:
                S = (g0 * ar + g1 * ag) + g2 * ab
                if bg is not None or gA is not None:
                    S = (S - gbg * aw) if defect != "S_without_bg" else S
                    S = S + gAr * aw
            if reg_k:
                Wt, Bt = W_carry, M_carry
                L = F(2.0) * _scan(lp)[63] + _scan(ls)[63] * (F(1.0) / F(3.0))
                S = S + F(2.0) * kq * L
                W_carry = M_carry = F(0.0)
            # sweep 2
            T_carry, P_carry = F(0.0), F(0.0)
            for b0 in range(0, npad, blk):
                step0 = b0 // (blk * blocks_per_step) * (blk * blocks_per_step)
                if b0 >= n:
                    break
                if b0 == step0 and b0 > 0:
                    if defect == "T_carry_step":
                        T_carry = F(0.0)
                    if defect == "P_carry_step":
                        P_carry = F(0.0)
                if defect == "P_carry_block" and b0 > 0:
                    P_carry = F(0.0)
                cc, ss, dd = data(b0, step0)
                x, Ti, exs, tot = weights(T_carry, cc, ss, dd)
                gc = [(((g0 * cc[p][:, 0] + g1 * cc[p][:, 1]) + g2 * cc[p][:, 2]) - gbg) + gAr if (bg is not None or gA is not None)
                      else (g0 * cc[p][:, 0] + g1 * cc[p][:, 1]) + g2 * cc[p][:, 2] for p in range(per)]
                a = [F(1.0) - exs[p] for p in range(per)]
                if reg_k:
                    i = b0 + per * lanes[None, :] + np.arange(per)[:, None]
                    w = [Ti[p] * a[p] for p in range(per)]
                    Wlt, Mlt, wm, wtot, mtot = prefixes(W_carry, M_carry, w, mm[i])
                    for p in range(per):
                        q = F(2.0) * (mm[i][p] * ((F(2.0) * Wlt[p] + w[p]) - Wt) - ((F(2.0) * Mlt[p] + wm[p]) - Bt)) + (F(2.0) / F(3.0)) * (w[p] * dwp[i][p])
                        gc[p] = gc[p] + kq * q
                    W_carry, M_carry = W_carry + wtot, M_carry + mtot
                wgc = [Ti[p] * a[p] * gc[p] for p in range(per)]
                if per == 1:
                    pincl = [P_carry + _scan(wgc[0])]
                    P_next = pincl[0][63]
                else:
                    pin = _scan(wgc[0] + wgc[1])
                    pincl1 = P_carry + pin
                    pincl = [pincl1 if defect == "pincl0_is_pincl1" else pincl1 - wgc[1], pincl1]
                    P_next = P_carry + pin[63]
                for p in range(per):
                    i = b0 + per * lanes + p
                    limit = n - per if defect == "short_mask" else n
                    act = (b0 + per * lanes) < limit
                    o = np.stack([g0 * Ti[p] * a[p], g1 * Ti[p] * a[p], g2 * Ti[p] * a[p],
                                  dd[p] * (Ti[p] * exs[p] * gc[p] - (S - pincl[p]))], 1).astype(np.float16)
                    out[s.start + i[act]] = o[act]
                T_carry = T_carry + tot
                P_carry = P_next
    return out


def emulate_compat(b, g, t_vals, defect=None):
    """fp32 restatement of volrender_bwd_compat_kernel (64 samples per step, t carried from step to step); defect
    "t_carry_step": the carry reset to 0 at every step"""
    out = np.full((b.N, 4), np.nan, np.float16)
    with np.errstate(over="ignore"):
        for r, s in enumerate(ray_slices(b)):
            n = s.stop - s.start
            if n == 0:
                continue
            c, sig, t = b.rad[s, :3], b.rad[s, 3], t_vals[s].astype(np.float32)
            tp = np.concatenate([[F(0.0)], t[:-1]]).astype(np.float32)
            if defect == "t_carry_step":
                tp[64::64] = 0.0
            g0, g1, g2 = (F(v) for v in g[r])
            delta = np.abs(t - tp)
            tr = delta * sig
            e = np.exp(-sig * delta)
            dg = F(0.0) + g0 * tr * c[:, 0] * delta * e
            dg = dg + g1 * tr * c[:, 1] * delta * e
            dg = dg + g2 * tr * c[:, 2] * delta * e
            om = F(1.0) - np.exp(-delta * sig)
            out[s] = np.stack([g0 * tr * om, g1 * tr * om, g2 * tr * om, dg], 1).astype(np.float16)
    return out


def compat_ulps(got, ref64):
    """distance in fp16 units of the last place between the stored values and half(float64)"""
    with np.errstate(over="ignore"):
        return np.abs(half_order(np.asarray(got, np.float16)) - half_order(ref64.astype(np.float16)))
