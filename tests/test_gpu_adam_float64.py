"""The Adam kernels of optimizer.hip against float64, without the oracle (tests/_adam_float64.py: the rules restated in numpy
float64 from include/rtxn.h, every bound derived there from the kernels' own roundings; tests/test_adam_float64_reference.py:
the CPU proof that the inputs and the bounds fit and that seeded defects fall outside).

  (a) one step from the device's own state over step counts 1 .. 70 000 (per-entry counts 0 .. 2^24 mixed inside quads), fp32
      gradients over 10^[-12 .. 6] and where g^2 underflows, fp16 subnormals and +-65504, +-0 beside non-zeros, both eps;
  (b) the bias-corrected rates alone against rho_dense / rho_sparse, for three beta pairs;
  (c) 600 free-running steps against a float64 trajectory that never sees the device, under the bounds carried as a recurrence;
  (d) every family whose walk differs at n = 1 .. 1025 and across the grid caps (the second grid-stride trip), n = 0;
  (e) one pointer at a time off its alignment: the same bits as the aligned run.
Every buffer is a view inside a larger allocation whose margins hold a sentinel; every test asserts the margins untouched.
No tolerance here is a literal: each comes from a function of the helper.  `pytest -m gpu -s` prints the figures recorded in
profiles/r20/adam_float64.txt."""
import numpy as np
import pytest

import _adam_float64 as A

pytestmark = pytest.mark.gpu

F32 = np.float32
MARGIN = 64                                   # elements on either side of a buffer: 128 or 256 bytes, so the view stays 16-byte aligned
PATTERN = {2: 0x5a5a, 4: 0x5a5a5a5a}
SPARSE_GLOBAL_T = 250                         # the step whose factor(t) the sparse option cases run under
EMA_D = 0.95


def _ibits(torch, x):
    return x.view({2: torch.int16, 4: torch.int32}[x.element_size()])


class Buf:
    """n elements that start MARGIN + shift elements into an allocation filled with a sentinel"""

    def __init__(self, torch, n, dtype, shift=0):
        self.torch, self.n, self.lo = torch, n, MARGIN + shift
        self.alloc = torch.empty(n + 2 * MARGIN + 16, dtype=dtype, device="cuda")
        self.pattern = PATTERN[self.alloc.element_size()]
        _ibits(torch, self.alloc).fill_(self.pattern)
        self.t = self.alloc[self.lo:self.lo + n]
        assert self.alloc.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (shift * self.alloc.element_size()) % 16

    def margins_untouched(self):
        a = _ibits(self.torch, self.alloc)
        return bool((a[:self.lo] == self.pattern).all()) and bool((a[self.lo + self.n:] == self.pattern).all())


NAMES = {"w": "float32", "m": "float32", "v": "float32", "p": "float16", "s": "int32", "acc": "float32", "stamps": "int32"}


class Dev:
    """the buffers of one optimizer state on the device; shifts: {name: elements off the 16-byte alignment}"""

    def __init__(self, torch, n, half, shifts=None):
        shifts = shifts or {}
        self.torch, self.n, self.half = torch, n, half
        self.b = {k: Buf(torch, n, getattr(torch, dt), shifts.get(k, 0)) for k, dt in NAMES.items()}
        self.b["g"] = Buf(torch, n, torch.float16 if half else torch.float32, shifts.get("g", 0))

    def __getattr__(self, k):
        return self.b[k].t

    def load(self, **arrays):
        for k, a in arrays.items():
            if not isinstance(a, self.torch.Tensor):
                a = np.ascontiguousarray(a)
                a = self.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)
            self.b[k].t.copy_(a)

    def read(self, names=("w", "m", "v", "p", "s", "g")):
        out = {k: self.b[k].t.cpu().numpy() for k in names}
        return {k: (a.view(np.uint32) if a.dtype == np.int32 else a) for k, a in out.items()}

    def margins_untouched(self):
        return all(b.margins_untouched() for b in self.b.values())


class Ctx:
    """what a step reads beside its buffers: the options with the rate kernel's outputs, and where asked the scaler's state (its
    multiplier word set by hand) and the EMA's"""

    def __init__(self, torch, api, sched=None, wd=0.0, multiplier=None, ema=False):
        self.torch, self.api = torch, api
        self.factor, self.guard = torch.zeros(1, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        self.step, self.rates = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
        self.opt = api.optimizer_options(sched, wd, multiplier is not None, self.factor, self.guard)
        self.scaler = self.ema = None
        if multiplier is not None:
            self.scaler_state = api.loss_scaler_state_tensor(api.loss_scaler())
            self.scaler_state.view(torch.float32)[1] = float(multiplier)
            self.scaler = api.loss_scaler(state=self.scaler_state, partials=api.loss_scaler_workspace())
        if ema:
            self.ema_state = torch.zeros(4, dtype=torch.int32, device="cuda")
            self.ema = api.weight_ema(EMA_D, state=self.ema_state)

    def set_step(self, t, h, table_lr=0.0):
        """the rate kernel at step t: returns factor(t) as stored; the rates are in self.rates"""
        self.step.fill_(t - 1)
        kw = dict(lr=h.lr, table_lr=table_lr, table_effective_lr=self.rates[1:2], beta1=h.b1, beta2=h.b2)
        if self.ema is not None:
            self.api.optimizer_rate_ema(self.opt, self.ema, self.step, self.rates[0:1], **kw)
        else:
            self.api.optimizer_rate(self.opt, self.step, self.rates[0:1], **kw)
        assert int(self.step.item()) == t and self.guard.tolist()[2] == 0
        return float(self.factor.item())

    def updates(self):
        return int(self.ema_state[0].item())


def _launch(api, form, D, ctx, h, loss_scale, zero, t=None):
    kw = dict(beta1=h.b1, beta2=h.b2, eps=h.eps)
    dense, sparse = (D.w, D.p, D.g, D.m, D.v), (D.w, D.p, D.g, D.m, D.v, D.s)
    if form == "step":
        (api.adam_step_half_grads if D.half else api.adam_step)(*dense, t, lr=h.lr, loss_scale=loss_scale, **kw)
    elif form == "captured":
        api.adam_step_captured(*dense, ctx.rates[0:1], loss_scale=loss_scale, zero_grads=zero, **kw)
    elif form == "opt":
        api.adam_step_opt(*dense, ctx.rates[0:1], ctx.opt, lr=h.lr, loss_scale=loss_scale, zero_grads=zero, **kw)
    elif form == "scaled":
        api.adam_step_scaled(*dense, ctx.rates[0:1], ctx.opt, ctx.scaler, lr=h.lr, zero_grads=zero, **kw)
    elif form == "ema":
        api.adam_step_ema(*dense, ctx.rates[0:1], ctx.opt, ctx.ema, D.acc, lr=h.lr, loss_scale=loss_scale, zero_grads=zero, **kw)
    elif form == "sparse":
        api.adam_step_sparse(*sparse, lr=h.lr, loss_scale=loss_scale, zero_grads=zero, **kw)
    elif form == "sparse_opt":
        api.adam_step_sparse_opt(*sparse, ctx.opt, lr=h.lr, loss_scale=loss_scale, zero_grads=zero, **kw)
    elif form == "sparse_scaled":
        api.adam_step_sparse_scaled(*sparse, ctx.opt, ctx.scaler, lr=h.lr, zero_grads=zero, **kw)
    elif form == "sparse_ema":
        api.adam_step_sparse_ema(*sparse, ctx.opt, ctx.ema, D.acc, D.stamps, lr=h.lr, loss_scale=loss_scale, zero_grads=zero, **kw)
    else:
        raise ValueError(form)


class Agg:
    """the largest err / bound and share above half of it over the cases of one test, per tensor"""

    def __init__(self):
        self.worst, self.half = {}, {}

    def add(self, res):
        for k, r in res.items():
            if isinstance(r, A.Result):
                self.worst[k], self.half[k] = max(self.worst.get(k, 0.0), r.worst), max(self.half.get(k, 0.0), r.half)

    def line(self, title):
        return f"measured {title}: err / bound " + ", ".join(f"{k} {self.worst[k]:.3f} ({self.half[k]:.4f} above half)" for k in self.worst)


# ------------------------------------------------------------------------------------------------------- (a) one step
A_FORMS = [(form, half, zero) for form in ("step", "captured", "opt", "scaled", "sparse", "sparse_opt", "sparse_scaled")
           for half in (False, True) for zero in (False, True) if not (form == "step" and zero)]          # the by-value step has no ZERO flag


@pytest.mark.parametrize("form,half,zero", A_FORMS, ids=[f"{f}-{'fp16' if h else 'fp32'}-{'zero' if z else 'keep'}" for f, h, z in A_FORMS])
def test_one_step_from_the_devices_own_state(gpu, form, half, zero):
    torch = gpu
    from rtx_nerf_amd import api
    sparse, opt, dev_factor = form.startswith("sparse"), form.split("_")[-1] in ("opt", "scaled"), form.endswith("scaled")
    cases = [c for c in A.a_cases() if (c.sparse, c.half, c.zero, c.opt) == (sparse, half, zero, opt)]
    assert len(cases) == (6 if sparse else len(A.T_DENSE))
    D, agg = Dev(torch, cases[0].n, half), Agg()
    for c in cases:
        h = A.hyper(A.LR, eps=c.eps, wd=A.WD if opt else 0.0)
        gf = float(F32(0.75) / F32(c.loss_scale)) if dev_factor else None               # a multiplier word with a clipping coefficient in it
        before, gf = A.case_inputs(c, gf=gf)
        ctx = Ctx(torch, api, A.SCHED if opt else None, h.wd, multiplier=gf if dev_factor else None)
        f = ctx.set_step(SPARSE_GLOBAL_T if sparse else c.t, h) if form != "step" else 1.0
        assert opt or f == 1.0
        D.load(**before)
        own = D.read()                                                                  # the state the step starts from, as the device holds it
        assert all(np.array_equal(A.bits(own[k]), A.bits(before[k])) for k in own)
        _launch(api, form, D, ctx, h, c.loss_scale, zero, t=c.t)
        got = D.read()
        rho = A.rho_dense(c.t, h.b1, h.b2, power_ulps=1.0) if form == "step" else None   # the by-value step's rate is the host's powf form
        ref = A.case_reference(c, own, own["g"], gf, f, h, dense_rho=rho)
        res = A.check_step(got, own, own["g"], ref, zero=zero, sparse=sparse)
        assert A.all_ok(res), (c, A.line(form, res))
        assert D.margins_untouched(), c
        agg.add(res)
    print(agg.line(f"one step {form} {'fp16' if half else 'fp32'} {'zero' if zero else 'keep'}"))


# ------------------------------------------------------------------------------------------------------- (b) the rates alone
RATE_STEPS = sorted(set(A.T_DENSE + [c + 1 for c in A.COUNTS_SPARSE]))


@pytest.mark.parametrize("betas", A.BETAS)
def test_rate_kernel_and_host_rate_against_float64(gpu, betas):
    torch = gpu
    from rtx_nerf_amd import api
    h = A.hyper(1e-3, b1=betas[0], b2=betas[1])
    tlr = float(F32(1e-2))
    ctx = Ctx(torch, api, A.SCHED)
    worst = [0.0, 0.0, 0.0]
    for t in RATE_STEPS:
        f = ctx.set_step(t, h, table_lr=tlr)
        assert abs(f - A.factor64(t, **A.SCHED)) <= A.factor_bound(f)                          # factor(t): double arithmetic, rounded once
        e, et = ctx.rates.tolist()
        rho = float(A.rho_dense(t, h.b1, h.b2))
        r, rt = A.rate64(h.lr * f, h.b1, h.b2, t), A.rate64(tlr * f, h.b1, h.b2, t)
        host, rho_host = api.adam_effective_lr(h.lr, h.b1, h.b2, t), float(A.rho_dense(t, h.b1, h.b2, power_ulps=1.0))
        errs = [abs(e - r) / r / rho, abs(et - rt) / rt / rho, abs(host - A.rate64(h.lr, h.b1, h.b2, t)) / A.rate64(h.lr, h.b1, h.b2, t) / rho_host]
        worst = [max(a, b) for a, b in zip(worst, errs)]
        assert max(errs) <= 1.0, (t, errs)
    r1 = float(A.rho_dense(1, h.b1, h.b2))
    print(f"measured dense rate betas {betas}: err / rho_dense lr_eff {worst[0]:.3f}, table_lr_eff {worst[1]:.3f}, rtxn_adam_effective_lr {worst[2]:.3f}"
          f" | rho_dense(1) = {r1:.3e}")


@pytest.mark.parametrize("betas", A.BETAS)
def test_sparse_in_kernel_rate_against_float64(gpu, betas):
    """w = 0, m = 0, v = 0, g = 1: the step leaves -w' = fl(fl(r m') / den), from which r is read back (recovered_rate_bound)"""
    torch = gpu
    from rtx_nerf_amd import api
    n = A.N_SPARSE
    h = A.hyper(A.LR, b1=betas[0], b2=betas[1], eps=1e-15)
    counts = A.sparse_counts(n, 0)
    D = Dev(torch, n, False)
    zeros = np.zeros(n, np.float32)
    D.load(w=zeros, m=zeros, v=zeros, p=zeros.astype(np.float16), s=counts, g=np.ones(n, np.float32))
    _launch(api, "sparse", D, None, h, 1.0, False)
    got = D.read()
    t = counts.astype(np.int64) + 1
    assert np.array_equal(got["s"].astype(np.int64), t) and D.margins_untouched()
    den = np.sqrt(got["v"]) + F32(h.eps)                                                 # fp32, as the kernel forms it
    rec = -got["w"].astype(np.float64) * den.astype(np.float64) / got["m"].astype(np.float64)
    ref, rho = A.rate64(h.lr, h.b1, h.b2, t), A.rho_sparse(t, h.b1, h.b2)
    err = abs(rec - ref) / ref
    assert (err <= A.recovered_rate_bound(rho)).all(), float((err / rho).max())
    k = int(np.argmax(err))
    print(f"measured sparse rate betas {betas}: largest relative error {err.max():.3e} at t = {t[k]} (rho_sparse there {rho[k]:.3e}), "
          f"largest err / rho_sparse {float((err / A.recovered_rate_bound(rho)).max()):.3f} | at t = 1: {err[t == 1].max():.3e} of rho_sparse(1) = {float(A.rho_sparse(1, h.b1, h.b2)):.3e}")


# ------------------------------------------------------------------------------------------------------- (c) a free run
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_free_run_against_a_float64_trajectory(gpu, sparse):
    torch = gpu
    from rtx_nerf_amd import api
    n = A.FREE_N
    h = A.hyper(A.LR, eps=1e-15 if sparse else 1e-8, wd=A.WD)
    gf = float(F32(1.0) / F32(A.FREE_LOSS_SCALE))
    w0 = (np.random.default_rng(9).standard_normal(n) * 0.1).astype(np.float32)
    run, D, ctx = A.FreeRun(w0, sparse, h, gf), Dev(torch, n, False), Ctx(torch, api, A.SCHED, h.wd)
    zeros = np.zeros(n, np.float32)
    D.load(w=w0, m=zeros, v=zeros, p=w0.astype(np.float16), s=np.zeros(n, np.uint32))
    for t in range(1, A.FREE_STEPS + 1):
        raw = A.free_run_gradient(t)
        D.load(g=raw)
        f = ctx.set_step(t, h)                                                           # the factor the kernels read: an input, not state
        _launch(api, "sparse_opt" if sparse else "opt", D, ctx, h, A.FREE_LOSS_SCALE, True)
        ref = run.step(raw, f)
        if t in A.FREE_RECORD:
            got = D.read()
            res = {k: A.compare(got[k], getattr(ref, k), getattr(ref, "b" + k)) for k in ("w", "m", "v")}
            print(A.line(f"free run {'sparse' if sparse else 'dense'} step {t}", res))
            assert A.all_ok(res)
            assert not got["g"].any() and np.array_equal(A.bits(got["p"]), A.bits(got["w"].astype(np.float16)))
            if sparse:
                assert np.array_equal(got["s"].astype(np.int64), ref.steps)
    assert D.margins_untouched()


# ------------------------------------------------------------------------------------------------------- (d) sizes
_BIG = {}


def _size_inputs(sparse, half, n):
    """inputs of one size; the large ones are made once per (walk, gradient type) and shared, with their reference"""
    key = (sparse, half, n)
    if n < 100_000 or key not in _BIG:
        c = A.size_case(sparse, half)
        before, gf = A.case_inputs(c, n, raw=A.big_sparse_gradient(half, c.seed) if sparse and n == A.SPARSE_BIG else None)
        before["acc"] = (np.random.default_rng(n).standard_normal(n) * 0.1).astype(np.float32)
        if n < 100_000:
            return [before, gf, None, before]
        import torch
        on_device = {k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for k, a in before.items()}
        _BIG[key] = [before, gf, None, on_device]                                       # uploaded once; every case copies from there
    return _BIG[key]


@pytest.mark.parametrize("zero", [False, True], ids=["keep", "zero"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("ema", [False, True], ids=["opt", "ema"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_every_walk_at_every_size(gpu, sparse, ema, half, zero):
    torch = gpu
    from rtx_nerf_amd import api
    form = ("sparse_" if sparse else "") + ("ema" if ema else "opt")
    c = A.size_case(sparse, half)
    h = A.hyper(A.LR, eps=c.eps, wd=A.WD)
    ctx, agg = Ctx(torch, api, A.SCHED, h.wd, ema=ema), Agg()
    t = SPARSE_GLOBAL_T if sparse else c.t
    for n in [0] + A.SMALL_SIZES + [A.SPARSE_BIG if sparse else A.DENSE_BIG]:
        f = ctx.set_step(t, h)
        D = Dev(torch, n, half)
        if n == 0:
            _launch(api, form, D, ctx, h, c.loss_scale, zero)                             # RTXN_OK (anything else raises), nothing written
            torch.cuda.synchronize()
            assert D.margins_untouched()
            continue
        shared = _size_inputs(sparse, half, n)
        before, gf = shared[0], shared[1]
        u = ctx.updates() if ema else 0
        before["stamps"] = np.full(n, u - 1 if ema and sparse else 0, np.uint32)          # current up to the update before: the lazy catch-up has no gap
        D.load(**shared[3])
        D.load(stamps=before["stamps"])
        _launch(api, form, D, ctx, h, c.loss_scale, zero)
        got = D.read(("w", "m", "v", "p", "s", "g", "acc", "stamps"))
        if shared[2] is None or shared[2][0] != f:
            shared[2] = (f, A.case_reference(c, before, before["g"], gf, f, h))
        ref = shared[2][1]
        res = A.check_step(got, before, before["g"], ref, zero=zero, sparse=sparse)
        sel = slice(None) if ref.sel is None else ref.sel
        if ema:
            want, bound = A.ema_bound(before["acc"][sel], ref.w, ref.bw, float(F32(EMA_D)))
            res["acc"] = A.compare(got["acc"][sel], want, bound)
            res["the average moves only where Adam did"] = A.kept_outside(got["acc"], before["acc"], sel)
            if sparse:
                res["stamps"] = bool((got["stamps"][sel] == u).all()) and A.kept_outside(got["stamps"], before["stamps"], sel)
            else:
                res["stamps"] = np.array_equal(got["stamps"], before["stamps"])
        else:
            res["no average without the EMA"] = np.array_equal(A.bits(got["acc"]), A.bits(before["acc"])) and np.array_equal(got["stamps"], before["stamps"])
        if not sparse:
            res["dense counts stay"] = np.array_equal(got["s"], before["s"])
        assert A.all_ok(res), (n, A.line(form, res))
        assert D.margins_untouched(), n
        if n >= 100_000:
            print(A.line(f"size {n} {form} {'fp16' if half else 'fp32'} {'zero' if zero else 'keep'}", res))
        else:
            agg.add(res)
        del D
    print(agg.line(f"sizes {A.SMALL_SIZES} {form} {'fp16' if half else 'fp32'} {'zero' if zero else 'keep'}"))


# ------------------------------------------------------------------------------------------------------- (e) alignment
def _variants(sparse, ema, half):
    """(what moves, by how many elements, whether the alignment predicate still holds)"""
    v = [("w", 1, False), ("m", 1, False), ("v", 1, False), ("p", 1, False), ("p", 4, True)]
    v += [("g", 4, False), ("g", 8, True)] if half else [("g", 1, False)]
    if sparse:
        v.append(("s", 1, False))
    if ema:
        v.append(("acc", 1, False))
        if sparse:
            v.append(("stamps", 1, False))
    return v


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("ema", [False, True], ids=["opt", "ema"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_one_pointer_at_a_time_off_its_alignment(gpu, sparse, ema, half):
    """ZERO is on: the sparse walk's gradient buffer then shows which path ran (the body clears a consumed quad whole, the
    scalar path leaves the -0.0 of a mixed quad), so 'the vector body is used on an 8-byte-aligned params' is an assertion"""
    torch = gpu
    from rtx_nerf_amd import api
    form = ("sparse_" if sparse else "") + ("ema" if ema else "opt")
    n = A.N_SPARSE
    c = A.size_case(sparse, half)
    h = A.hyper(A.LR, eps=c.eps, wd=A.WD)
    before, gf = A.case_inputs(c, n)
    before["acc"] = (np.random.default_rng(5).standard_normal(n) * 0.1).astype(np.float32)
    ctx = Ctx(torch, api, A.SCHED, h.wd, ema=ema)
    t = SPARSE_GLOBAL_T if sparse else c.t
    names = ("w", "m", "v", "p", "s", "g", "acc", "stamps")

    def run(shifts):
        f = ctx.set_step(t, h)
        D = Dev(torch, n, half, shifts)
        before["stamps"] = np.full(n, ctx.updates() - 1 if ema and sparse else 0, np.uint32)
        D.load(**before)
        _launch(api, form, D, ctx, h, c.loss_scale, True)
        got = D.read(names)
        assert D.margins_untouched(), shifts
        return f, got

    f, base = run({})
    ref = A.case_reference(c, before, before["g"], gf, f, h)
    res = A.check_step(base, before, before["g"], ref, zero=True, sparse=sparse, vec=True)
    assert A.all_ok(res), A.line(form, res)
    print(A.line(f"aligned {form} {'fp16' if half else 'fp32'}", res))
    for name, shift, vec in _variants(sparse, ema, half):
        f2, got = run({name: shift})
        assert f2 == f
        for k in names:
            if k == "stamps" and ema and sparse:
                assert np.array_equal(got[k] != before["stamps"], base[k] != base[k].min()), (name, shift, k)   # stamped with the update's own number
            elif k != "g":
                assert np.array_equal(A.bits(got[k]), A.bits(base[k])), (name, shift, k)
        assert np.array_equal(A.bits(got["g"]), A.grads_after(before["g"], True, sparse, vec)), (name, shift, "gradient buffer")
