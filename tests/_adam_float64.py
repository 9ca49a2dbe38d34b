"""Float64 restatement of the Adam rules of include/rtxn.h, the bounds a faithful fp32 kernel stays inside, the inputs the GPU tests
feed the kernels and an fp32 stand-in of the two walks (a helper module, not a conftest; numpy only, no oracle, no project code).

THE RULES (every value is the one the kernel reads: gradients as stored in fp16 / fp32, beta1, beta2, eps, lr, weight_decay as the
float32 the ABI passes, the factor on the raw gradient -- 1 / loss_scale or the scaler's multiplier word -- as float32, factor(t)
as the float32 the rate kernel stored; all of them exact in float64):
    g = raw gf
    m' = b1 m + (1 - b1) g          v' = b2 v + (1 - b2) g^2          w' = w - r_t m' / (sqrt(v') + eps)
    r_t = lr_t sqrt(1 - b2^t) / (1 - b1^t),   lr_t = lr f
    w'' = w' - (lr_t wd) w'                    the decoupled decay, behind the Adam update
  sparse rule: an element whose gradient is +-0 keeps every word of its state; the entry's own count advances where Adam applied
  and is the t of its rate; the decay applies only there.

THE BOUNDS.  u = 2^-24; gamma(k) = k u / (1 - k u) bounds k roundings that multiply.  No constant here comes from running a
kernel; each function below derives its own in its docstring: rho_dense, rho_sparse (the relative error of a bias-corrected
rate), step_reference (one step from given state, with the errors the state came in with -- zeros for one step, the recurrence
for a free run), ema_bound.

THE STAND-IN.  standin_step() is the two walks op by op in numpy float32 (numpy rounds every operation and fuses none, as the
file's -ffp-contract=off build does): the alignment predicate's vector / tail split, the grid-stride trips, the quad zero test,
exp2 with the kernel's argument.  tests/test_adam_float64_reference.py shows on the CPU that it stays inside every bound on
every input set the GPU tests use, and that each seeded DEFECT falls outside an assertion the GPU tests make.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126                      # the smallest normal fp32
F32 = np.float32
THREADS = 256
DENSE_BLOCKS, SPARSE_BLOCKS = 4096, 8192


def gamma(k):
    return k * U / (1.0 - k * U)


Hyper = namedtuple("Hyper", "lr b1 b2 eps wd")


def hyper(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
    """the float32 values the ABI passes, held as Python floats (exact)"""
    return Hyper(*(float(F32(x)) for x in (lr, b1, b2, eps, wd)))


# ------------------------------------------------------------------------------------------------------- the rates
def pow64(b, t):
    return np.power(np.float64(b), np.asarray(t, np.float64))


def rate64(lr_t, b1, b2, t):
    """r_t = lr_t sqrt(1 - b2^t) / (1 - b1^t) in float64"""
    return lr_t * np.sqrt(1.0 - pow64(b2, t)) / (1.0 - pow64(b1, t))


def half_ulp(p):
    """half the spacing of fp32 at p (p >= 0): 2^(floor(log2 p) - 24), the subnormal spacing 2^-150 below 2^-126"""
    p = np.asarray(p, np.float64)
    e = np.floor(np.log2(np.maximum(p, TINY)))
    return np.exp2(e - 24.0)


def _rate_error(t, b1, b2, E1, E2, c):
    """the expression both rate forms share, (lr f) * sqrtf(1 - p2) / (1 - p1), with |p - b^t| <= E:
        lr f                      one rounding                                                    u
        1 - p2                    one rounding (exact where p2 >= 1/2; counted all the same)      u       } under the root:
        the error of p2           E2 / (1 - b2^t)                                                         } halved
        sqrtf                     correctly rounded                                               u
        the product               one rounding                                                    u
        1 - p1                    one rounding, and E1 / (1 - b1^t)                               u
        the quotient              correctly rounded                                               u
    c = 1 + 1/2 + 1 + 1 + 1 + 1 = 5.5 roundings, first order; the factor (1 + 16 u) covers the products of these terms."""
    assert c == 5.5
    q1, q2 = 1.0 - pow64(b1, t), 1.0 - pow64(b2, t)
    return (c * U + 0.5 * E2 / q2 + E1 / q1) * (1.0 + 16 * U)


def rho_dense(t, b1, b2, power_ulps=0.5):
    """Relative error of the dense rate, rate_update of optimizer.hip: p = (float)pow((double)b, (double)t) is b^t correctly rounded,
    |p - b^t| <= half an ulp of fp32 at b^t; then _rate_error's expression:
        rho_dense(t) = u (5.5 + (1/2) h(b2^t) / (u (1 - b2^t)) + h(b1^t) / (u (1 - b1^t))),   h = half_ulp
    (for b^t in [1/2, 1) h = u / 2: the familiar u (5.5 + b2^t / (4 (1 - b2^t)) + b1^t / (2 (1 - b1^t))) with b^t ~ 1).
    power_ulps = 1: rtxn_adam_effective_lr, whose powf is within one ulp of b^t, not half of one."""
    t = np.asarray(t, np.float64)
    return _rate_error(t, b1, b2, 2.0 * power_ulps * half_ulp(pow64(b1, t)), 2.0 * power_ulps * half_ulp(pow64(b2, t)), 5.5)


def rho_sparse(t, b1, b2):
    """Relative error of the sparse rule's in-kernel rate, adam_sparse_rate: p = v_exp_f32(fl((float)t fl(log2 b))).
        the instruction           1 ulp of its result (the ISA guide's figure), and results below 2^-126 are flushed:   2 h(b^t) + 2^-126
        the argument              log2 b rounded once on the host (u), (float)t exact below 2^24 (one more u from there on),
                                  the product rounded once (u): |arg - t log2 b| <= k u |t log2 b|, k = 2 (3 from 2^24 on);
                                  d(2^x) = 2^x ln 2 dx:                                          b^t ln 2 k u |t log2 b|
        E(t; b) = 2 h(b^t) + 2^-126 + b^t ln 2 k u t |log2 b|, the second order of the argument's term included by the factor
        exp(ln 2 k u t |log2 b|); then _rate_error's expression with E1 = E(t; b1), E2 = E(t; b2).
    At t = 1 and beta2 = 0.999 this is 3.0e-5: one ulp of 0.999 against 1 - 0.999, halved by the root."""
    t = np.asarray(t, np.float64)

    def E(b):
        p, arg = pow64(b, t), t * abs(np.log2(b))
        d = np.log(2.0) * np.where(t < 2.0 ** 24, 2.0, 3.0) * U * arg
        return 2.0 * half_ulp(p) + TINY + p * d * np.exp(np.minimum(d, 1.0))
    return _rate_error(t, b1, b2, E(b1), E(b2), 5.5)


def recovered_rate_bound(rho):
    """The sparse rate is read back from a step with w = 0: w' = -fl(fl(r m') / den) exactly (0 - q is exact), with m' and
    den = fl(fl(sqrt(v')) + eps) known bit for bit from the device's own m' and v'.  So -w' den / m' is r within the product's
    and the quotient's rounding:  (1 + rho)(1 + u)^2 - 1"""
    return (1.0 + np.asarray(rho, np.float64)) * (1.0 + U) ** 2 - 1.0


# ------------------------------------------------------------------------------------------------------- one step in float64
Ref = namedtuple("Ref", "w m v steps touched bw bm bv upd sel", defaults=(None,))


def step_reference(w, m, v, raw, gf, h, rate, rho, decay, touched=None, steps=None, E=(0.0, 0.0, 0.0)):
    """One Adam step in float64 from the state (w, m, v) and the bound of a faithful fp32 kernel beside it.
    raw: the stored gradient; gf: the float32 factor on it (raw gf is exact in float64); rate: r_t in float64 (one number or one
    per element); rho: its relative error bound; decay: lr_t wd in float64 (0: the kernel executes no decay).  touched: where
    the sparse rule applies Adam (None: everywhere); elsewhere the state is returned as it came, with its incoming error.
    E = (E_w, E_m, E_v): what the fp32 state may differ from (w, m, v) by on entry; zeros for a step from the device's own state.

    adam_one as written, every operation rounded once and none fused:
      g  = fl(raw gf)                                    1 rounding; raw gf is kept normal by the inputs, so it is relative
      m' = fl(fl(b1 m) + fl(fl(1 - b1) g))               A = b1 m: the product and the sum, 2; B = (1 - b1) g: fl(1 - b1), g, the
                                                         product and the sum, 4:   |m' - ref| <= gamma(4) (|A| + |B|) + b1 E_m (1 + gamma(4))
      v' = fl(fl(b2 v) + fl(fl(fl(1 - b2) g) g))         B = (1 - b2) g g: fl(1 - b2), g twice, two products and the sum, 6:
                                                         |v' - ref| <= gamma(6) (|A| + |B|) + 2^-126 + b2 E_v (1 + gamma(6));
                                                         the absolute term: a product below the normal range loses up to the
                                                         spacing there, or all of itself in a build that flushes
      s  = fl(sqrt(v'))                                  |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= min(e_v / sqrt(v_ref), sqrt(e_v)),
                                                         then 1 rounding: d_s = that + u sqrt(v_ref)
      den = fl(s + eps)                                  d = d_s + u (den_ref + d_s);    |1 / den - 1 / den_ref| <= kappa / den_ref, kappa = d / (den_ref - d)
      q  = fl(fl(r m') / den)                            r within rho, the product, the quotient:   R = (1 + rho)(1 + kappa)(1 + u)^2 - 1
                                                         |q - upd| <= |upd| R + r e_m / den_ref (1 + R)
      w1 = fl(w - q)                                     e_1 = E_w + e_q + u (|w1_ref| + E_w + e_q)
      w2 = fl(w1 - fl(fl(fl(lr f) wd) w1))               exactly w1 (1 - decay) carries e_1 (1 - decay): the incoming error CONTRACTS; the
                                                         decay's own two roundings and the product's: gamma(3) decay (|w1_ref| + e_1);
                                                         the difference's rounding: u (|w2_ref| + e_1);  (1 + 8 u) for their products:
                                                         e_2 = e_1 (1 - decay) + (gamma(3) decay (|w1_ref| + e_1) + u (|w2_ref| + e_1)) (1 + 8 u)
    which is the shape u |ref| + k_w u |update| + rho |update| plus the propagated m' and v' terms."""
    f64 = np.float64
    w, m, v = (np.asarray(a).astype(f64) for a in (w, m, v))
    n = w.size
    E_w, E_m, E_v = (np.broadcast_to(np.asarray(e, f64), (n,)) for e in E)
    g = np.asarray(raw).astype(f64) * f64(gf)
    rate, rho = np.broadcast_to(np.asarray(rate, f64), (n,)), np.broadcast_to(np.asarray(rho, f64), (n,))
    with np.errstate(all="ignore"):
        A_m, B_m = h.b1 * m, (1.0 - h.b1) * g
        m1 = A_m + B_m
        e_m = gamma(4) * (abs(A_m) + abs(B_m)) + h.b1 * E_m * (1.0 + gamma(4))
        A_v, B_v = h.b2 * v, (1.0 - h.b2) * g * g
        v1 = A_v + B_v
        e_v = gamma(6) * (abs(A_v) + abs(B_v)) + TINY + h.b2 * E_v * (1.0 + gamma(6))
        s = np.sqrt(v1)
        d_s = np.minimum(np.where(s > 0, e_v / np.where(s > 0, s, 1.0), np.inf), np.sqrt(e_v)) + U * s
        den = s + h.eps
        d = d_s + U * (den + d_s)
        assert (d < den).all(), "the denominator's error reaches the denominator: eps is too small for these inputs"
        kappa = d / (den - d)
        upd = rate * m1 / den
        R = (1.0 + rho) * (1.0 + kappa) * (1.0 + U) ** 2 - 1.0
        e_q = abs(upd) * R + abs(rate) * e_m / den * (1.0 + R)
        w1 = w - upd
        e_1 = E_w + e_q + U * (abs(w1) + E_w + e_q)
        if decay != 0.0:
            w2 = w1 - decay * w1
            assert 0.0 < decay < 1.0
            e_2 = e_1 * (1.0 - decay) + (gamma(3) * decay * (abs(w1) + e_1) + U * (abs(w2) + e_1)) * (1.0 + 8 * U)
        else:
            w2, e_2 = w1, e_1
    if touched is None:
        touched = np.ones(n, bool)
    st = None if steps is None else np.asarray(steps).astype(np.int64) + touched
    return Ref(np.where(touched, w2, w), np.where(touched, m1, m), np.where(touched, v1, v), st, touched,
               np.where(touched, e_2, E_w), np.where(touched, e_m, E_m), np.where(touched, e_v, E_v), np.where(touched, upd, 0.0))


def ema_bound(s, w2, e_w, d):
    """s' = fl(fl(d s) + fl(fl(1 - d) w'')) of the _ema kernels (the lazy form with gap 0 returns s itself from the catch-up):
    reference d s + (1 - d) w2 in float64 with d the float32; A = d s: the product and the sum, 2; B = (1 - d) w: fl(1 - d), the
    product and the sum, 3; w'' itself within e_w:    |s' - ref| <= gamma(3) (|A| + |B|) + (1 - d) e_w (1 + gamma(3))"""
    A, B = d * np.asarray(s, np.float64), (1.0 - d) * w2
    return A + B, gamma(3) * (abs(A) + abs(B)) + (1.0 - d) * e_w * (1.0 + gamma(3))


# ------------------------------------------------------------------------------------------------------- the checker
Result = namedtuple("Result", "bad worst half")     # elements NOT inside the bound; largest err / bound; share above half of it


def compare(got, ref, bound):
    """Counts the elements not inside the bound (a NaN or an Inf counts like any other wrong value; no element is left out)"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(ref) == np.shape(bound), (got.dtype, got.shape, np.shape(ref))
    with np.errstate(all="ignore"):
        err = abs(got.astype(np.float64) - ref)
        inside = err <= bound
        err = np.where(np.isfinite(err), err, np.inf)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    if ratio.size == 0:
        return Result(0, 0.0, 0.0)
    return Result(int((~inside).sum()), float(ratio.max()), float((ratio > 0.5).mean()))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def kept_outside(got, before, moved):
    """True where every element outside `moved` (indices or a mask) holds the bits it held before"""
    x = bits(got) ^ bits(before)
    x[moved] = 0
    return not x.any()


def factor_bound(f):
    """factor(t) is formed in double and rounded to float once: u |f|, and as much again for the double arithmetic's own
    last digits differing between two libms; 2^-149: the spacing of fp32 where the factor is subnormal"""
    return 2.0 * U * abs(f) + 2.0 ** -149


def grads_after(raw, zero, sparse, vec):
    """The gradient buffer behind a step, bit for bit.  Without ZERO: untouched.  Dense ZERO: all zero words.  Sparse ZERO: what
    the walk consumes is cleared -- in the vector body a quad that is not all +-0 whole, in the tail (every element, without the
    alignment) an element that is not +-0 -- and what it passes over keeps its bits, the sign of a -0.0 among them."""
    b = bits(raw).copy()
    if not zero:
        return b
    if not sparse:
        return np.zeros_like(b)
    n = b.size
    n4 = n // 4 if vec else 0
    nz = (raw != 0)
    quad = nz[:4 * n4].reshape(-1, 4).any(axis=1).repeat(4)
    clear = np.concatenate([quad, nz[4 * n4:]])
    b[clear] = 0
    return b


def check_step(got, before, raw, ref, *, zero, sparse, vec=True):
    """Every assertion the GPU tests make on one step.  got / before: dicts of numpy arrays -- w, m, v (float32), p (float16), g (the
    gradient buffer behind the step) and, sparse, s (the update counts).  Returns {name: Result or bool}; all_ok() judges it."""
    sel = slice(None) if ref.sel is None else ref.sel         # ref.sel: the entries a sparse reference was formed for
    out = {k: compare(got[k][sel], getattr(ref, k), getattr(ref, "b" + k)) for k in ("w", "m", "v")}
    with np.errstate(over="ignore"):
        out["params are fp16(master)"] = np.array_equal(bits(got["p"]), bits(got["w"].astype(np.float16)))
    out["gradient buffer"] = np.array_equal(bits(got["g"]), grads_after(raw, zero, sparse, vec))
    if sparse:
        out["update counts"] = np.array_equal(got["s"][sel].astype(np.int64) & 0xffffffff, ref.steps)
        out["skipped entries keep their bits"] = all(kept_outside(got[k], before[k], sel if ref.sel is not None else ref.touched) for k in ("w", "m", "v", "p", "s"))
    return out


def all_ok(res):
    return all((r.bad == 0) if isinstance(r, Result) else bool(r) for r in res.values())


def line(title, res):
    """One line per case for the log and the record"""
    parts = [f"{k} {r.worst:.3f} ({r.half:.4f} above half)" for k, r in res.items() if isinstance(r, Result)]
    wrong = [k for k, r in res.items() if (r.bad if isinstance(r, Result) else not r)]
    return f"measured {title}: err / bound " + ", ".join(parts) + (f" | FAILED: {wrong}" if wrong else " | ok")


# ------------------------------------------------------------------------------------------------------- the inputs
T_DENSE = [1, 2, 3, 10, 100, 693, 6_931, 70_000]
COUNTS_SPARSE = [0, 1, 2, 9, 99, 692, 6_930, 99_999, 2 ** 24]
N_DENSE, N_SPARSE = 4 * 64 * 3 + 3, 4_099
EPS = [1e-8, 1e-15]
LOSS_SCALES = [1.0, 128.0, 2.0 ** 15]
BETAS = [(0.9, 0.99), (0.9, 0.999), (0.9, 0.9999)]
LR, WD = 1e-2, 0.05
SCHED = dict(kind="cosine", warmup_steps=40, decay_start=100, decay_steps=600, ratio=0.1)      # 1/40 .. 1, then down to 0.1 and flat: never 0


def factor64(t, kind="constant", warmup_steps=0, decay_start=0, decay_steps=1, ratio=1.0, staircase=False):
    """include/rtxn.h's factor(t) in float64; the ratio is the float32 the struct holds"""
    warm = min(1.0, t / warmup_steps) if warmup_steps > 0 else 1.0
    x = max(0, t - decay_start) / decay_steps
    if staircase:
        x = np.floor(x)
    r = float(F32(ratio))
    dec = 1.0 if kind == "constant" else r ** x if kind == "exponential" else r + (1.0 - r) * (1.0 + np.cos(np.pi * min(x, 1.0))) / 2.0
    return warm * dec


def gradients(n, half, sparse, loss_scale, seed):
    """The stored gradient of n elements (n >= 64 for the planted quads; any n otherwise) whose scaled value raw / loss_scale is
      fp32: normal x 10^[-12 .. 6], and one element in sixteen in the band 1e-25 .. 1e-20, where g^2 lies below 2^-126;
      fp16: normal x 0.3 with the smallest subnormal (2^-24) and +-65504 sprinkled in;
    with +-0 planted beside non-zeros: quad 5 all +0, quad 9 (-0, x, -0, y), quad 13 only +-0, the tail's first element -0.0 and
    (sparse) about half of the rest zero.  Every non-zero scaled gradient stays a normal fp32, so raw gf is rounded relatively."""
    rng = np.random.default_rng(seed)
    if half:
        g = (rng.standard_normal(n) * 0.3).astype(np.float16)
        g[g == 0] = np.float16(0.25)
        k = rng.integers(0, 8, n)
        g[k == 0] = np.float16(2.0 ** -24) * np.where(rng.uniform(size=(k == 0).sum()) < 0.5, -1, 1).astype(np.float16)
        g[k == 1] = np.float16(65504.0) * np.where(rng.uniform(size=(k == 1).sum()) < 0.5, -1, 1).astype(np.float16)
    else:
        x = rng.standard_normal(n)
        x[abs(x) < 1e-3] = 0.5
        scaled = x * 10.0 ** rng.integers(-12, 7, n)
        band = rng.integers(0, 16, n) == 0
        scaled[band] = np.sign(x[band]) * 10.0 ** rng.uniform(-25, -20, band.sum())
        g = (scaled * loss_scale).astype(np.float32)
    if sparse:
        g[rng.uniform(size=n) < 0.5] = 0
    if n >= 64:
        a, b = g.dtype.type(0.25), g.dtype.type(-0.5)
        g[20:24] = 0
        g[36:40] = np.array([-0.0, a, -0.0, b], g.dtype)
        g[52:56] = np.array([-0.0, 0.0, -0.0, -0.0], g.dtype)
    if n % 4 and n > 1:
        g[4 * (n // 4)] = -0.0
        if n % 4 > 1:
            g[4 * (n // 4) + 1] = g.dtype.type(0.375)
    nz = g[g != 0].astype(np.float64) / loss_scale
    assert nz.size == 0 or (abs(nz).min() >= TINY and np.isfinite(g).all())
    return g


def start_state(n, raw, gf, kind, seed):
    """(w, m, v) in float32.  'history': v about g^2, m about g, random signs (1e-3 where the gradient is zero, so that a skipped
    entry has state to keep); 'zeros': the first step of a run."""
    rng = np.random.default_rng(seed + 1000)
    w = (rng.standard_normal(n) * 0.1).astype(np.float32)
    if kind == "zeros":
        return w, np.zeros(n, np.float32), np.zeros(n, np.float32)
    g = abs(raw.astype(np.float64) * float(F32(gf)))
    g[g == 0] = 1e-3
    with np.errstate(over="ignore", under="ignore"):
        v = (g * g * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        m = (g * rng.uniform(0.3, 1.0, n) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)).astype(np.float32)
    assert np.isfinite(v).all() and np.isfinite(m).all()
    return w, m, v


def sparse_counts(n, seed):
    """per-entry update counts from COUNTS_SPARSE, mixed so that the four lanes of a quad carry four different rates"""
    c = np.array(COUNTS_SPARSE, np.int64)
    idx = (np.arange(n) + np.arange(n) // 4 * 3 + seed) % len(c)
    return c[idx].astype(np.uint32)


Case = namedtuple("Case", "sparse half zero opt k n t eps loss_scale state seed")


def a_cases():
    """The one-step cases of the GPU test (a): both walks, both gradient types, ZERO on and off, with and without the options; k
    runs over the step counts (dense) or six variants (sparse) and cycles eps, the loss scale and the starting state."""
    out = []
    for sparse in (False, True):
        for half in (False, True):
            for zero in (False, True):
                for opt in (False, True):
                    for k in range(len(T_DENSE) if not sparse else 6):
                        out.append(Case(sparse, half, zero, opt, k, N_SPARSE if sparse else N_DENSE, None if sparse else T_DENSE[k],
                                        EPS[k % 2], LOSS_SCALES[k % 3], ("history", "zeros")[(k // 2) % 2],
                                        7 + 64 * sparse + 32 * half + 16 * zero + 8 * opt + k))
    return out


def case_inputs(c, n=None, raw=None, gf=None):
    """{w, m, v, g, s, p} of a Case in numpy, and gf: the float32 factor on the raw gradient (1 / loss_scale unless one is given,
    as the scaler's multiplier word is); raw: a gradient to use in place of the case's own"""
    n = c.n if n is None else n
    gf = float(F32(1.0) / F32(c.loss_scale)) if gf is None else float(F32(gf))
    g = gradients(n, c.half, c.sparse, c.loss_scale, c.seed) if raw is None else raw
    w, m, v = start_state(n, g, gf, c.state, c.seed)
    s = sparse_counts(n, c.seed) if c.sparse else np.zeros(n, np.uint32)
    with np.errstate(over="ignore"):
        return dict(w=w, m=m, v=v, g=g, s=s, p=w.astype(np.float16)), gf


def case_reference(c, before, raw, gf, f32_factor, h=None, dense_rho=None):
    """step_reference of a Case from `before` (what the device, or the stand-in, started from).  f32_factor: factor(t) as stored
    (1 without the options).  dense_rho: the dense rate's bound where it is not rho_dense(t) (the by-value step's powf)."""
    h = h or hyper(LR, eps=c.eps, wd=WD if c.opt else 0.0)
    lr_t = h.lr * float(F32(f32_factor))
    decay = lr_t * h.wd
    if c.sparse:
        sel = np.flatnonzero(raw != 0)              # the sparse rule moves these alone: the reference is formed for them, the rest keep their bits
        t = before["s"][sel].astype(np.int64) + 1
        return step_reference(before["w"][sel], before["m"][sel], before["v"][sel], raw[sel], gf, h, rate64(lr_t, h.b1, h.b2, t),
                              rho_sparse(t, h.b1, h.b2), decay, steps=before["s"][sel])._replace(sel=sel)
    rho = rho_dense(c.t, h.b1, h.b2) if dense_rho is None else dense_rho
    return step_reference(before["w"], before["m"], before["v"], raw, gf, h, rate64(lr_t, h.b1, h.b2, c.t), rho, decay)


# ------------------------------------------------------------------------------------------------------- the free run of (c)
FREE_STEPS, FREE_N, FREE_LOSS_SCALE, FREE_RECORD = 600, 4_099, 128.0, (1, 10, 100, 600)
TOUCH = [1.0, 0.5, 0.1, 0.01]


def free_run_gradient(step, seed=77):
    """The stored fp32 gradient of step `step` (1-based) of the free run: entry i is touched with probability TOUCH[i % 4], entries
    with i % 16 == 15 not before step 500; magnitudes normal x 0.3 x 10^-(i % 7) after scaling by 1 / FREE_LOSS_SCALE"""
    n, rng = FREE_N, np.random.default_rng(seed * 100_000 + step)
    i = np.arange(n)
    x = rng.standard_normal(n)
    x[abs(x) < 1e-3] = 0.5
    g = (x * 0.3 * 10.0 ** -(i % 7) * FREE_LOSS_SCALE).astype(np.float32)
    g[rng.uniform(size=n) >= np.array(TOUCH)[i % 4]] = 0
    if step < 500:
        g[i % 16 == 15] = 0
    return g


class FreeRun:
    """The float64 trajectory from a start w0 (moments and counts zero), and beside it the one-step bounds carried forward as a
    recurrence: step_reference with E = the bounds of the step before.  The m and v errors contract with b1 and b2, the w error
    sums and contracts by 1 - decay; a skipped entry carries state and error over unchanged.  Never sees the device's state."""

    def __init__(self, w0, sparse, h, gf):
        n = w0.size
        self.sparse, self.h, self.gf, self.t = sparse, h, gf, 0
        self.w, self.m, self.v = w0.astype(np.float64), np.zeros(n), np.zeros(n)
        self.E = (np.zeros(n), np.zeros(n), np.zeros(n))
        self.steps = np.zeros(n, np.int64)

    def step(self, raw, f32_factor):
        h = self.h
        self.t += 1
        lr_t = h.lr * float(F32(f32_factor))
        if self.sparse:
            t = self.steps + 1
            ref = step_reference(self.w, self.m, self.v, raw, self.gf, h, rate64(lr_t, h.b1, h.b2, t), rho_sparse(t, h.b1, h.b2), lr_t * h.wd,
                                 touched=raw != 0, steps=self.steps, E=self.E)
            self.steps = ref.steps
        else:
            ref = step_reference(self.w, self.m, self.v, raw, self.gf, h, rate64(lr_t, h.b1, h.b2, self.t), rho_dense(self.t, h.b1, h.b2),
                                 lr_t * h.wd, E=self.E)
        self.w, self.m, self.v, self.E = ref.w, ref.m, ref.v, (ref.bw, ref.bm, ref.bv)
        return ref


# ------------------------------------------------------------------------------------------------------- the sizes of (d)
DENSE_BIG = 4 * 256 * DENSE_BLOCKS + 4 * 512 + 3
SPARSE_BIG = 4 * 256 * SPARSE_BLOCKS + 4 * 512 + 3
SMALL_SIZES = [1, 2, 3, 4, 5, 7, 1_023, 1_024, 1_025]


def size_case(sparse, half):
    """the Case the size and alignment runs are made from: options on, ZERO on, eps 1e-8, loss scale 128, state with a history"""
    return [c for c in a_cases() if (c.sparse, c.half, c.zero, c.opt, c.k) == (sparse, half, True, True, 4)][0]


def big_sparse_gradient(half, seed):
    """SPARSE_BIG elements, 1 % non-zero: in the first trip of the grid-stride loop (its first 64 quads all zero), in the second
    trip (quads 0 .. 63 of its 512 all zero, the last vector quad not), and all three tail elements."""
    n, rng = SPARSE_BIG, np.random.default_rng(seed)
    dt = np.float16 if half else np.float32
    g = np.zeros(n, dt)
    first = 4 * 256 * SPARSE_BLOCKS
    idx = rng.choice(np.arange(256, first), size=n // 100, replace=False)
    g[idx] = (rng.standard_normal(idx.size) * 0.3 + np.where(rng.uniform(size=idx.size) < 0.5, -1, 1)).astype(dt)
    second = np.arange(first + 256, first + 2048)
    pick = second[rng.uniform(size=second.size) < 0.3]
    g[pick] = dt(0.5)
    g[first + 2044:first + 2048] = np.array([0.25, -0.0, -1.5, 0.0], dt)
    g[n - 3:] = np.array([-0.75, 0.125, 2.0], dt)
    assert not g[:256].any() and not g[first:first + 256].any() and (g[idx] != 0).all()
    return g


# ------------------------------------------------------------------------------------------------------- the fp32 stand-in
DEFECTS = ["bias_correction_at_t_minus_1", "g_not_squared", "eps_inside_sqrt", "coupled_decay", "decay_with_corrected_rate",
           "betas_swapped_in_rate", "inv_loss_scale_twice", "sparse_decays_skipped_moments", "sparse_global_count",
           "quad_skipped_on_first_zero", "second_trip_dropped", "tail_starts_one_late", "sparse_rate_off_1e-4"]


def dense_grid(n):
    return min(DENSE_BLOCKS, ((n + 3) // 4 + THREADS - 1) // THREADS)


def sparse_grid(n):
    return max(1, min(SPARSE_BLOCKS, (n // 4 + THREADS - 1) // THREADS))


def standin_dense_rate(lr, f, b1, b2, t, defect=None):
    """rate_update: powers in double rounded once, then fp32"""
    lr, f, b1, b2 = F32(lr), F32(f), F32(b1), F32(b2)
    if defect == "bias_correction_at_t_minus_1":
        t = t - 1
    if defect == "betas_swapped_in_rate":
        b1, b2 = b2, b1
    p2, p1 = F32(np.float64(b2) ** np.float64(t)), F32(np.float64(b1) ** np.float64(t))
    with np.errstate(all="ignore"):
        return (lr * f) * np.sqrt(F32(1) - p2) / (F32(1) - p1)


def _exp2_f32(x, shift):
    """2^x for fp32 x: float64's, rounded to fp32 (flushed below 2^-126, as the instruction does).  shift = +-1: moved one ulp up /
    down wherever that keeps it within ONE ulp of 2^x -- the worst the instruction's stated accuracy allows on that side"""
    with np.errstate(all="ignore"):
        exact = np.exp2(x.astype(np.float64))
        p = exact.astype(np.float32)
    p = np.where(p < F32(TINY), F32(0), p).astype(np.float32)
    if shift:
        q = np.nextafter(p, F32(2.0 if shift > 0 else 0.0)).astype(np.float32)
        ok = (p > 0) & (abs(q.astype(np.float64) - exact) <= 2.0 * half_ulp(exact))
        p = np.where(ok, q, p).astype(np.float32)
    return p


def standin_sparse_rate(lr_t, st, b1, b2, defect=None, exp_shift=0, global_t=None):
    """adam_sparse_rate: log2 beta rounded once on the host, t = (float)st, one exp2 each"""
    l1, l2 = F32(np.log2(np.float64(F32(b1)))), F32(np.log2(np.float64(F32(b2))))
    if defect == "betas_swapped_in_rate":
        l1, l2 = l2, l1
    st = np.asarray(st, np.int64)
    if defect == "bias_correction_at_t_minus_1":
        st = st - 1
    if defect == "sparse_global_count":
        st = np.full_like(st, global_t)
    t = st.astype(np.float32)
    with np.errstate(all="ignore"):
        r = F32(lr_t) * np.sqrt(F32(1) - _exp2_f32(t * l2, exp_shift)) / (F32(1) - _exp2_f32(t * l1, exp_shift))
    if defect == "sparse_rate_off_1e-4":
        r = r * F32(1.0 + 1e-4)
    return r.astype(np.float32)


def visited(n, sparse, vec, defect=None):
    """(body, tail): which elements the vector body and the scalar tail of a walk reach -- four elements per lane where the
    alignment predicate holds, grid-stride trips of grid x 256 lanes, the tail from 4 n4"""
    n4 = n // 4 if vec else 0
    stride = (sparse_grid(n) if sparse else dense_grid(n)) * THREADS
    body, tail = np.zeros(n, bool), np.zeros(n, bool)
    quads = n4 if defect != "second_trip_dropped" else min(n4, stride)
    body[:4 * quads] = True
    start = 4 * n4 + (1 if defect == "tail_starts_one_late" else 0)
    tail[start:n if defect != "second_trip_dropped" else min(n, start + stride)] = True
    return body, tail


def standin_step(before, raw, gf, h, *, sparse, zero, f32_factor=1.0, t=None, vec=True, defect=None, exp_shift=0, rate=None):
    """One step of either walk in numpy float32, op by op.  before: {w, m, v, p, s}; raw: the stored gradient; gf: the float32
    factor on it; h: Hyper; t: the step (dense); rate: the dense rate as a float32 where it does not come from the rate kernel.
    Returns the same dict behind the step, with g: the gradient buffer behind it."""
    n = raw.size
    w, m, v, p, s = (before[k].copy() for k in ("w", "m", "v", "p", "s"))
    b1, b2, eps, lr, wd, gf = F32(h.b1), F32(h.b2), F32(h.eps), F32(h.lr), F32(h.wd), F32(gf)
    lr_t = lr * F32(f32_factor)
    decay = lr_t * wd
    body, tail = visited(n, sparse, vec, defect)
    g_left = raw.copy()
    with np.errstate(all="ignore"):
        g = raw.astype(np.float32) * gf
        if defect == "inv_loss_scale_twice":
            g = g * gf
        if sparse:
            rawnz = (bits(raw) & (0x7fff if raw.dtype == np.float16 else 0x7fffffff)) != 0
            n4 = n // 4 if vec else 0
            quad_live = rawnz[:4 * n4].reshape(-1, 4).any(axis=1) if defect != "quad_skipped_on_first_zero" else rawnz[:4 * n4].reshape(-1, 4)[:, 0]
            live = np.concatenate([quad_live.repeat(4), g[4 * n4:] != 0])       # body: the quad's test on the raw words; tail: g == 0
            consumed = (body | tail) & live
            if zero:
                g_left[consumed] = 0
            apply = consumed & (g != 0)                                         # rule.one returns at g == 0
            s = s.astype(np.int64)
            s[apply] += 1
            r = standin_sparse_rate(lr_t, s, h.b1, h.b2, defect, exp_shift, global_t=int(s.max()))
            s = (s & 0xffffffff).astype(np.uint32)
        else:
            apply = body | tail
            if zero:
                g_left[apply] = 0
            r = standin_dense_rate(lr, f32_factor, b1, b2, t, defect) if rate is None else F32(rate)
        if defect == "coupled_decay":
            g = g + wd * w
        m1 = b1 * m + (F32(1) - b1) * g
        v1 = b2 * v + ((F32(1) - b2) * g if defect == "g_not_squared" else (F32(1) - b2) * g * g)
        den = np.sqrt(v1 + eps) if defect == "eps_inside_sqrt" else np.sqrt(v1) + eps
        w1 = w - r * m1 / den
        if defect == "decay_with_corrected_rate":
            w1 = w1 - (r * wd) * w1
        elif decay != 0 and defect != "coupled_decay":
            w1 = w1 - decay * w1
        w, m, v = (np.where(apply, a, o).astype(np.float32) for a, o in ((w1, w), (m1, m), (v1, v)))
        if defect == "sparse_decays_skipped_moments":
            m, v = np.where(apply, m, b1 * m).astype(np.float32), np.where(apply, v, b2 * v).astype(np.float32)
        p = np.where(apply, w.astype(np.float16), p)
    return dict(w=w, m=m, v=v, p=p, s=s, g=g_left)
