"""The multiresolution hash grid restated in numpy float64 from tiny-cuda-nn's published formulas (grid.h), with DERIVED error
bounds per encoded element and per table entry.  Nothing here imports the project's CPU oracle or its kernels: the oracle is
written by the same hands as the kernels, so "HIP == oracle" passes a shared misreading; this module is the second opinion.
tests/test_hashgrid_float64_reference.py runs it without a GPU (against the oracle, the closed-form golden file and seeded
defects), tests/test_gpu_hashgrid_float64.py holds the kernels to it.

Geometry (all float32, as tcnn's host code):   scale_l = exp2f(l * log2f(s)) * base - 1,   res_l = ceil(scale_l) + 1,
size_l = min(res_l^3 rounded up to 8, 2^T) entries, levels back to back.  exp2f / log2f are taken as correctly rounded (float64
numpy, rounded once to float32; the CPU test compares with the C library's).  A level is stored densely when res^3 <= size.

Encode of x in [-1, 1]^3:   x01 = x / 2 + 1 / 2,  pos = x01 * scale + 1 / 2,  g = floor(pos),  fr = pos - g,  trilinear weights
w_c = prod_a (c_a ? fr_a : 1 - fr_a) over the eight corners q = g + c, entry index  q0 + q1 r + q2 r^2  (dense) or
q0 ^ (q1 * 2654435761) ^ (q2 * 805459861) in 32-bit arithmetic (hashed), BOTH reduced % size;  ref = sum_c w_c t[index_c].

THE ENCODE BOUND (u = 2^-24; per sample, level and feature), three terms:
  1. the kernel rounds its fp32 sum to fp16 once: half an fp16 ulp of ref, subnormals kept (floor 2^-25);
  2. fp32 arithmetic on exact inputs: a weight is a product of three factors fr or 1 - fr (up to three subtractions and two
     products: <= 5 u relative), the fused multiply-add forms w t without a rounding of its own, and the eight accumulations are
     sequential: the first is exact against 0, the j-th rounds a partial sum of magnitude <= sum_{c <= j} w_c |t_c| once.  A term
     therefore sits through 5 + (at most) 7 roundings -- 12 u sum w|t| if every one of them took its full half ulp in the same
     direction and all the weight lay on the first corner.  The bound charges 8 u sum w|t|, the figure the scatter's run sum is
     charged as well: tighter than that worst case (for a table of U(-1, 1) either is hundreds of times smaller than term 1);
  3. the position: x01 = fma(x, 1/2, 1/2) is rounded to fp32 (<= 2^-25 absolute, x01 <= 1), pos = fma(x01, scale, 1/2) once more
     (<= 2^-24 (scale + 1/2)); together  dfr <= scale 2^-25 + (scale + 1/2) 2^-24 < (scale + 1) 2^-23  per axis; fr = pos - floor(pos)
     is exact.  The interpolant is multilinear inside a cell: |d ref / d fr_a| <= max - min of the eight corner values, so a
     sample FARTHER than tau_l = 4 (scale_l + 1) 2^-23 from every face of its cell (fp32 and float64 then agree on the cell) moves
     by at most 3 dfr (max - min).  NEARER than tau_l fp32 may floor into the neighbouring cell: the interpolant is continuous
     across the face, but the slope on the far side is the neighbour's, of which only |slope| <= 2 max|table of the level| is
     known: 3 dfr 2 max|t_l|.

THE SCATTER BOUNDS (per table entry e and feature;  A_e = sum w |d| over the contributions (sample, corner) that reach e,
n_e their number,  pos_e = sum |d| 3 (scale + 1) 2^-23  since |dw / dfr_a| <= 1 for each of the three axes):
  fp32 atomics      (2 + 8 + n_e) u A_e + pos_e     2: weight and product roundings beyond the scan's; 8: the wave's segmented
                                                    scan, at most 7 dependent adds + the product (C_SCATTER of
                                                    tests/test_gpu_deterministic_gradients.py); n_e: one rounding per float
                                                    atomic, in whatever order they arrive, each partial sum <= A_e
  packed fp16       (n_e + 1) (2^-11 A_e + 2^-25) + pos_e     one rounding to fp16 per atomic and one per conversion of the run
                                                    sum, each max(2^-11 |v|, 2^-25): below 2^-14 fp16 is spaced 2^-24 apart.
                                                    (Without the 2^-25 the form cannot be met: the correctly rounded fp16 of
                                                    the EXACT sum already misses it on entries whose only contribution has a
                                                    weight near 0 -- tests/test_hashgrid_float64_reference.py shows it.)
  deterministic     2 u |sum| + 8 u A_e + n 2^-41 + pos_e      (the fixed-point shadow: _scatter_bound of the same test file)
A (sample, level) pair NEARER than tau_l to a face may scatter into the neighbouring cell's corners in fp32 -- entries the
float64 sum never touches, by up to |d| -- so the scatter tests zero the gradient of such pairs (near_face()), at most 2 % of a
case's pairs (asserted by the callers); the encode tests keep them (continuity).  Entries with n_e = 0 have bound 0: exactly 0.

Direction features: sin(pi 2^f x + ph pi / 2) in float64.  DESIGN section 4 states <= 1 fp16 ulp per octave; the kernel reduces
the argument exactly in turns (fract(x 2^(f-1))) but ADDS ph / 4 in fp32 -- one rounding of a number below 1.25, <= 2^-24 turns,
2 pi 2^-24 in the value -- which is the whole error budget where the cosine crosses zero, so the phase-1 features carry that
term beside the ulp.  The term is needed, not convenient: directions_fp32_phase() gives that kernel an EXACT sine and still
leaves the bare ulp behind at zero crossings of the cosine (tests/test_hashgrid_float64_reference.py asserts it; the figures
of both, and of the kernels against the bare ulp, are in profiles/r16/hashgrid_float64.txt).
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
P1, P2 = 2654435761, 805459861
M32 = np.uint64(0xFFFFFFFF)

Level = namedtuple("Level", "scale res size offset hashed")        # scale: the float32 value as a Python float; offset in entries
Encoded = namedtuple("Encoded", "ref bound near half_ulp acc pos")  # [n, L * F] float64 (near: [n, L] bool)
Scattered = namedtuple("Scattered", "sum A n pos")                  # [n_entries * F]

# the sweep of the issue: (levels, F, T, base, s)
SWEEP = [
    (16, 2, 19, 16, 1.5),    # the bench grid: finest res 7007, res^3 > 2^32
    (4, 2, 4, 8, 2.0),       # all hashed, 16-entry levels, the smallest T
    (3, 2, 24, 2, 2.0),      # all dense, odd level count
    (2, 2, 24, 2, 2.0),      # all dense, even level count (the fused inference kernel takes it)
    (2, 2, 12, 16, 1.0),     # res^3 == 2^T exactly, two identical levels
    (3, 1, 10, 1, 2.0),      # F = 1, a res = 1 level (scale 0), odd level count
    (5, 1, 10, 4, 1.7),      # F = 1, odd, mixed dense and hashed
    (2, 8, 12, 8, 2.0),      # F = 8
    (16, 4, 14, 4, 1.5),     # F = 4, E = 80
    (6, 2, 12, 4, 1.6),      # mixed; a non-integer fp32 scale 5.4000001
]
DEFECTS = ["prime", "swap_yz", "no_half", "floor_res", "hashed_late", "no_wrap", "swap_feat", "no_round8", "rtz"]


def level_scale(l, base, s):
    lg = np.float32(np.log2(np.float64(np.float32(s))))                      # log2f
    p = np.float32(np.exp2(np.float64(np.float32(l) * lg)))                  # exp2f of the float32 product
    return float(np.float32(p * np.float32(base)) - np.float32(1.0))


def geometry(n_levels, T, base, s, defect=None):
    levels, off = [], 0
    for l in range(n_levels):
        scale = level_scale(l, base, s)
        res = int(np.floor(scale) if defect == "floor_res" else np.ceil(scale)) + 1
        dense = res ** 3 if defect == "no_round8" else (res ** 3 + 7) // 8 * 8
        size = min(dense, 1 << T)
        levels.append(Level(scale, res, size, off, res ** 3 > size))
        off += size
    if defect == "hashed_late":                                               # the decision of the level before
        levels = [lv._replace(hashed=levels[l - 1].hashed if l else False) for l, lv in enumerate(levels)]
    return levels


def n_entries(levels):
    return levels[-1].offset + levels[-1].size


def level_offsets(levels, F):
    """What HashGrid.level_offset(0 .. n_levels) returns: parameters before each level, then the total."""
    return [lv.offset * F for lv in levels] + [n_entries(levels) * F]


def tau(lv):
    return 4.0 * (lv.scale + 1.0) * 2.0 ** -23


def _cell(lv, x_f32, defect=None):
    x01 = np.asarray(x_f32, np.float32).astype(np.float64)[:, :3] * 0.5 + 0.5
    pos = x01 * lv.scale + (0.0 if defect == "no_half" else 0.5)
    g = np.floor(pos)
    return g.astype(np.int64), pos - g


def _corners(lv, g, fr, total, defect=None):
    """weights [n, 8] and GLOBAL entry indices [n, 8] (corner c: bit a of c chooses g_a + 1)"""
    n = g.shape[0]
    w = np.ones((n, 8))
    q = np.empty((3, n, 8), np.uint64)
    for c in range(8):
        for a in range(3):
            hi = (c >> a) & 1
            w[:, c] *= fr[:, a] if hi else 1.0 - fr[:, a]
            q[a, :, c] = (g[:, a] + hi).astype(np.uint64)
    r = np.uint64(lv.res)
    if lv.hashed:
        p1 = np.uint64(P1 + 1 if defect == "prime" else P1)
        idx = (q[0] & M32) ^ ((q[1] * p1) & M32) ^ ((q[2] * np.uint64(P2)) & M32)
    elif defect == "swap_yz":
        idx = q[0] + q[2] * r + q[1] * r * r
    else:
        idx = q[0] + q[1] * r + q[2] * r * r
    red = idx % np.uint64(lv.size)
    if defect == "no_wrap":                               # the +1 corner of a boundary cell keeps its unreduced index
        past = (q[0] >= r) | (q[1] >= r) | (q[2] >= r)
        red = np.where(past, idx, red)
    return w, ((red + np.uint64(lv.offset)) % np.uint64(total)).astype(np.int64)


def near_face(levels, x_f32):
    """[n, L] bool: the sample sits nearer than tau_l to a face of its level-l cell (on some axis)"""
    out = np.zeros((np.asarray(x_f32).shape[0], len(levels)), bool)
    for l, lv in enumerate(levels):
        _, fr = _cell(lv, x_f32)
        out[:, l] = (np.minimum(fr, 1.0 - fr) < tau(lv)).any(axis=1)
    return out


def half_ulp16(ref):
    """half the spacing of fp16 at |ref| (subnormals kept: never below 2^-25)"""
    a = np.abs(ref)
    _, e = np.frexp(a)                                    # |ref| = m 2^e, m in [1/2, 1): spacing 2^(e - 11)
    return np.where(a == 0, 2.0 ** -25, np.maximum(np.ldexp(1.0, e - 12), 2.0 ** -25))      # frexp(0) has e = 0: not 2^-12


def encode(levels, F, table_f16, x_f32, defect=None):
    """Hash features [n, L * F] in float64 with the bound of the module docstring, term by term."""
    x = np.asarray(x_f32, np.float32)
    n, L = x.shape[0], len(levels)
    total = n_entries(levels)
    tab = np.asarray(table_f16, np.float16).astype(np.float64).reshape(-1, F)
    if defect == "swap_feat":
        tab = tab[:, ::-1]
    ref, acc, pos = (np.zeros((n, L * F)) for _ in range(3))
    near = np.zeros((n, L), bool)
    for l, lv in enumerate(levels):
        g, fr = _cell(lv, x, defect)
        w, idx = _corners(lv, g, fr, total, defect)
        t = tab[np.minimum(idx, tab.shape[0] - 1)]        # [n, 8, F] (the minimum only matters to a defective geometry)
        sl = slice(l * F, (l + 1) * F)
        ref[:, sl] = np.einsum("nc,ncf->nf", w, t)
        acc[:, sl] = 8 * U * np.einsum("nc,ncf->nf", w, np.abs(t))
        near[:, l] = (np.minimum(fr, 1.0 - fr) < tau(lv)).any(axis=1)
        lo, hi = lv.offset, lv.offset + lv.size
        slope = np.where(near[:, l, None], 2.0 * np.abs(tab[lo:hi]).max(), t.max(axis=1) - t.min(axis=1))
        pos[:, sl] = 3.0 * (lv.scale + 1.0) * 2.0 ** -23 * slope
    hu = half_ulp16(ref)
    return Encoded(ref, hu + acc + pos, near, hu, acc, pos)


def directions(n_dir_freqs, dirs_f32):
    """(ref, bound) [n, 4 * n_dir_freqs]: dimension-major, frequency, (sin, cos), as the encoders lay them out"""
    d = np.asarray(dirs_f32, np.float32).astype(np.float64)
    ref = np.zeros((d.shape[0], 4 * n_dir_freqs))
    bound = np.zeros_like(ref)
    j = 0
    for a in range(2):
        for f in range(n_dir_freqs):
            for ph in range(2):
                ref[:, j] = np.sin(np.pi * np.ldexp(d[:, a], f) + ph * (np.pi / 2))
                bound[:, j] = 2 * half_ulp16(ref[:, j]) + ph * 2 * np.pi * U
                j += 1
    return ref, bound


def directions_bare_bound(ref):
    """1 fp16 ulp of ref and nothing else: what DESIGN section 4 stated before.  Reported beside the bound, never asserted."""
    return 2 * half_ulp16(ref)


def directions_fp32_phase(n_dir_freqs, dirs_f32):
    """The BEST a kernel can do that reduces the argument exactly in turns but adds the phase in fp32, as sin_turns() does:
    fract(x 2^(f-1)) exactly, + ph / 4 rounded once to fp32, then an EXACT sine rounded once to fp16.  [n, 4 * n_dir_freqs]."""
    d = np.asarray(dirs_f32, np.float32)
    out = np.zeros((d.shape[0], 4 * n_dir_freqs), np.float16)
    j = 0
    for a in range(2):
        for f in range(n_dir_freqs):
            t = np.ldexp(d[:, a], f - 1)                                  # exact in fp32 (no overflow at these sizes)
            t = (t - np.floor(t)).astype(np.float32)                      # exact but for a negative t above -2^-24 (-> 1.0)
            for ph in range(2):
                turns = (t + np.float32(0.25 * ph)).astype(np.float32)    # the one rounding
                out[:, j] = np.sin(2 * np.pi * turns.astype(np.float64)).astype(np.float16)
                j += 1
    return out


def scatter(levels, F, x_f32, denc_f16, defect=None):
    """Table gradient per entry and feature in float64: sum, A = sum w |d|, the contribution count and the positional term.
    denc_f16: [n, >= L * F] sample-major."""
    x = np.asarray(x_f32, np.float32)
    d = np.asarray(denc_f16, np.float16).astype(np.float64)
    total = n_entries(levels)
    out = Scattered(np.zeros(total * F), np.zeros(total * F), np.zeros(total * F, np.int64), np.zeros(total * F))
    for l, lv in enumerate(levels):
        g, fr = _cell(lv, x, defect)
        w, idx = _corners(lv, g, fr, total, defect)
        k = 3.0 * (lv.scale + 1.0) * 2.0 ** -23
        lo = int(idx.min())
        flat = (idx - lo).ravel()
        span = int(flat.max()) + 1
        for f in range(F):
            col = l * F + (F - 1 - f if defect == "swap_feat" else f)
            df = d[:, col]
            live = np.broadcast_to((df != 0)[:, None], w.shape).ravel()
            wd = (w * df[:, None]).ravel()
            dst = slice(lo * F + f, (lo + span) * F + f, F)
            out.sum[dst] += np.bincount(flat, wd, span)
            out.A[dst] += np.bincount(flat, np.abs(wd), span)
            out.n[dst] += np.bincount(flat, live.astype(np.float64), span).astype(np.int64)
            out.pos[dst] += np.bincount(flat, np.broadcast_to(np.abs(df)[:, None] * k, w.shape).ravel(), span)
    return out


def scatter_bound(sc, form, n_atomics=0):
    if form == "fp32":
        return (2 + 8 + sc.n) * U * sc.A + sc.pos
    if form == "fp16":
        return (sc.n + 1) * (2.0 ** -11 * sc.A + np.where(sc.n > 0, 2.0 ** -25, 0.0)) + sc.pos
    if form == "fp16 without the subnormal floor":        # reported beside the bound, never asserted
        return (sc.n + 1) * 2.0 ** -11 * sc.A + sc.pos
    if form == "float64":                                  # a double sum of fp32 weights rounded once to fp32 (the CPU oracle)
        return (2 + 8) * U * sc.A + sc.pos
    assert form == "deterministic"
    return 2 * U * np.abs(sc.sum) + 8 * U * sc.A + n_atomics * 2.0 ** -41 + sc.pos


# ------------------------------------------------------------------------------------------------ the assertions, shared
def check_encode(enc, got_f16):
    """got_f16 [n, L * F] against the bound, per element.  Returns (largest err / bound, share equal to fp16(ref), failures).
    A failure is an element NOT inside its bound, so a NaN or an infinity counts (and makes the ratio NaN or inf)."""
    got = np.asarray(got_f16, np.float16)
    err = np.abs(got.astype(np.float64) - enc.ref)
    ratio = err / enc.bound
    equal = float((got == enc.ref.astype(np.float16)).mean())
    return float(ratio.max()), equal, int((~(err <= enc.bound)).sum())


def check_scatter(sc, got, form, n_atomics=0):
    """got [n_entries * F] (any float type) against the bound of `form`, per entry: entries the reference leaves at zero (n = 0)
    have a zero bound.  Returns (largest err / bound over the touched entries, failures).  A failure is an entry NOT inside its
    bound: a NaN or an infinity counts, in a touched entry or an untouched one."""
    g = np.asarray(got).astype(np.float64)
    bound = scatter_bound(sc, form, n_atomics)
    if form == "deterministic":
        bound = np.where(sc.n > 0, bound, 0.0)
    err = np.abs(g - sc.sum)
    hit = bound > 0
    ratio = float((err[hit] / bound[hit]).max()) if hit.any() else 0.0
    return ratio, int((~(err <= bound)).sum())


def to_half(x64, defect=None):
    """float64 -> fp16, round to nearest even; "rtz": toward zero (the seeded conversion defect)"""
    h = np.asarray(x64, np.float64).astype(np.float16)
    if defect != "rtz":
        return h
    over = np.abs(h.astype(np.float64)) > np.abs(x64)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)


# ------------------------------------------------------------------------------------------------ the inputs, shared
def case_segments(levels, seed, P=300):
    """P one-segment rays (start, end, view) in [-1, 1]^3.  The first 64 + 3 L start on special points -- REGULAR sampling puts
    sample 0 exactly on the start --: 64 lattice points (multiples of 1/8, the corners +-1 among them) and, per level, the float32
    nearest a cell face with its two nextafter neighbours.  Some segments end exactly on a face of the cube."""
    rng = np.random.default_rng(seed)
    sp = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    lattice = (rng.integers(-8, 9, (64, 3)) / 8.0).astype(np.float32)
    lattice[0], lattice[1], lattice[2], lattice[3] = (-1, -1, -1), (1, 1, 1), (1, -1, 0.125), (0, 1, -1)
    k = 64
    sp[:k] = lattice
    for l, lv in enumerate(levels):
        if lv.scale > 0:
            face = int(rng.integers(1, max(2, int(lv.scale))))                # pos = face on axis a
            x = np.float32(2.0 * ((face - 0.5) / lv.scale) - 1.0)
            a = l % 3
            for v in (np.nextafter(x, np.float32(-2)), x, np.nextafter(x, np.float32(2))):
                sp[k, a] = v
                k += 1
    assert k <= P
    ep = np.clip(sp + rng.uniform(-0.06, 0.06, (P, 3)).astype(np.float32), -1, 1).astype(np.float32)
    for i in range(8):                                                        # ends on a face of [-1, 1]^3
        ep[P - 1 - i, i % 3] = 1.0 if i & 1 else -1.0
    view = np.stack([rng.uniform(0, 3.1, P), rng.uniform(-3.1, 3.1, P)], 1).astype(np.float32)
    return sp, ep, view


def case_table(levels, F, seed):
    rng = np.random.default_rng(seed + 1000)
    return rng.uniform(-1, 1, n_entries(levels) * F).astype(np.float16)


def case_live(n_levels, P=300):
    """[P] bool: 70 % of the segments live, the special points and both ends of the batch among them"""
    live = np.random.default_rng(n_levels).random(P) < 0.7
    live[[0, P - 1]] = True
    live[:64 + 3 * n_levels] = True
    return live


def case_gradient(levels, F, x_f32, seed, live=None):
    """denc [n, L * F] fp16 ~ N(0, 1/4), rows of dead segments zero, near-face (sample, level) pairs zero.  Returns it with the
    share of pairs zeroed for nearness."""
    rng = np.random.default_rng(seed + 2000)
    n, L = x_f32.shape[0], len(levels)
    d = (rng.standard_normal((n, L * F)) * 0.5).astype(np.float16)
    if live is not None:
        d.reshape(n // 32, 32, L * F)[~live] = 0
    near = near_face(levels, x_f32)
    d.reshape(n, L, F)[near] = 0
    return d, float(near.mean())
