"""The CPU proof beside tests/test_gpu_adam_float64.py: an fp32 stand-in of the two Adam walks (tests/_adam_float64.py, op by op as
optimizer.hip writes them) stays inside every float64 bound on every input set the GPU tests use, with no element excluded, and
each seeded defect falls outside an assertion the GPU tests make.  So the inputs and the bounds fit together, and the bounds can
tell.  Runs without a GPU; the figures it prints stand beside the MI355X's in profiles/r20/adam_float64.txt."""
import numpy as np
import pytest

import _adam_float64 as A

F32 = np.float32
SPARSE_GLOBAL_T = 250            # the step whose factor(t) the sparse option cases run under


def _factor(c):
    return float(F32(A.factor64(c.t if not c.sparse else SPARSE_GLOBAL_T, **A.SCHED))) if c.opt else 1.0


def _run_case(c, defect=None, exp_shift=0, n=None, vec=True, raw=None):
    before, gf = A.case_inputs(c, n, raw)
    raw = before["g"]
    h = A.hyper(A.LR, eps=c.eps, wd=A.WD if c.opt else 0.0)
    f = _factor(c)
    got = A.standin_step(before, raw, gf, h, sparse=c.sparse, zero=c.zero, f32_factor=f, t=c.t, vec=vec, defect=defect, exp_shift=exp_shift)
    ref = A.case_reference(c, before, raw, gf, f, h)
    return A.check_step(got, before, raw, ref, zero=c.zero, sparse=c.sparse, vec=vec), got


def _worst(acc, res):
    for k, r in res.items():
        if isinstance(r, A.Result):
            acc[k] = max(acc.get(k, 0.0), r.worst)


# ------------------------------------------------------------------------------------------------------- the rates
@pytest.mark.parametrize("betas", A.BETAS)
def test_standin_rates_stay_inside_rho(betas):
    b1, b2 = (float(F32(b)) for b in betas)
    lr = float(F32(A.LR))
    ts = np.array(sorted(set(A.T_DENSE + [c + 1 for c in A.COUNTS_SPARSE])), np.int64)
    dense = np.array([A.standin_dense_rate(lr, 1.0, b1, b2, int(t)) for t in ts], np.float64)
    ref = A.rate64(lr, b1, b2, ts)
    e = abs(dense - ref) / ref
    rho = A.rho_dense(ts, b1, b2)
    print(f"stand-in rates, betas {betas}: dense max err {e.max():.3e} (rho {rho[np.argmax(e / rho)]:.3e}, err / rho {max(e / rho):.3f})")
    assert (e <= rho).all()
    for shift in (-1, 0, 1):
        sp = A.standin_sparse_rate(lr, ts, b1, b2, exp_shift=shift).astype(np.float64)
        e = abs(sp - ref) / ref
        rho = A.rho_sparse(ts, b1, b2)
        k = int(np.argmax(e))
        print(f"  sparse, exp2 moved {shift:+d} ulp: max err {e.max():.3e} at t = {ts[k]} (rho there {rho[k]:.3e}), err / rho {max(e / rho):.3f}")
        assert (e <= rho).all()


def test_rho_sparse_at_the_default_betas_is_the_ulp_of_beta2():
    """the figure the header quotes: 3.0e-5 at t = 1, and below 1e-4 exactly while 1 - beta2 >= about 3e-4"""
    assert 2.9e-5 < float(A.rho_sparse(1, *A.hyper(b1=0.9, b2=0.999)[1:3])) < 3.2e-5
    assert float(A.rho_sparse(1, *A.hyper(b1=0.9, b2=0.9996)[1:3])) < 1e-4 < float(A.rho_sparse(1, *A.hyper(b1=0.9, b2=0.9999)[1:3]))
    assert float(A.rho_dense(1, *A.hyper()[1:3])) < 1.6e-5


def test_host_rate_function_stays_inside_rho_dense():
    """rtxn_adam_effective_lr is host code: powf, then the same expression (no device needed)"""
    from rtx_nerf_amd import api
    for betas in A.BETAS:
        b1, b2 = (float(F32(b)) for b in betas)
        worst = 0.0
        for t in A.T_DENSE:
            got, ref = api.adam_effective_lr(A.LR, betas[0], betas[1], t), A.rate64(float(F32(A.LR)), b1, b2, t)
            e, rho = abs(got - ref) / ref, float(A.rho_dense(t, b1, b2, power_ulps=1.0))
            worst = max(worst, e / rho)
            assert e <= rho, (betas, t, e, rho)
        print(f"host rtxn_adam_effective_lr, betas {betas}: largest err / rho_dense(powf) {worst:.3f}")


# ------------------------------------------------------------------------------------------------------- one step
def test_standin_stays_inside_every_bound_on_every_one_step_input():
    worst = {}
    for c in A.a_cases():
        for shift in ((-1, 0, 1) if c.sparse else (0,)):
            res, _ = _run_case(c, exp_shift=shift)
            assert A.all_ok(res), (c, shift, A.line("stand-in", res))
            _worst(worst, res)
    print("stand-in, one step, largest err / bound over all cases:", {k: round(v, 3) for k, v in worst.items()})
    assert 0.0 < worst["w"] <= 1.0 and 0.0 < worst["m"] <= 1.0 and 0.0 < worst["v"] <= 1.0


def test_inputs_cover_what_they_are_there_for():
    g32, g16 = A.gradients(A.N_SPARSE, False, True, 128.0, 3), A.gradients(A.N_SPARSE, True, True, 2.0 ** 15, 4)
    s = g32.astype(np.float64) / 128.0
    assert ((s != 0) & (s * s < A.TINY)).any() and abs(s).max() > 1e5 and abs(s[s != 0]).min() < 1e-20
    assert (abs(g16) == np.float16(65504)).any() and (abs(g16) == np.float16(2.0 ** -24)).any()
    for g in (g32, g16):
        assert np.signbit(g[36]) and g[36] == 0 and g[37] != 0 and not g[52:56].any() and np.signbit(g[52])
        assert np.signbit(g[A.N_SPARSE - 3]) and g[A.N_SPARSE - 2] != 0
    counts = A.sparse_counts(A.N_SPARSE, 1).reshape(-1)[:4096].reshape(-1, 4)
    assert set(np.unique(counts)) == set(A.COUNTS_SPARSE) and (np.array([len(set(q)) for q in counts]) == 4).mean() > 0.5


# ------------------------------------------------------------------------------------------------------- sizes, alignment
@pytest.mark.parametrize("sparse", [False, True])
def test_standin_stays_inside_the_bounds_at_every_size(sparse):
    for c in (A.size_case(sparse, False), A.size_case(sparse, True)):            # the cases the GPU size runs are made from
        for n in A.SMALL_SIZES:
            res, _ = _run_case(c, n=n)
            assert A.all_ok(res), (c, n, A.line("stand-in", res))
        n = A.SPARSE_BIG if sparse else A.DENSE_BIG
        res, _ = _run_case(c, n=n, raw=A.big_sparse_gradient(c.half, c.seed) if sparse else None)
        print(A.line(f"stand-in n = {n} {'sparse' if sparse else 'dense'} half={c.half}", res))
        assert A.all_ok(res)


@pytest.mark.parametrize("sparse", [False, True])
def test_scalar_path_of_the_standin_is_the_vector_path_bit_for_bit(sparse):
    for c in [c for c in A.a_cases() if c.sparse == sparse and c.k == 1] + [A.size_case(sparse, False), A.size_case(sparse, True)]:
        n = A.N_SPARSE                                                           # the alignment runs of the GPU test: both walks at 4099
        (res_v, got_v), (res_s, got_s) = _run_case(c, vec=True, n=n), _run_case(c, vec=False, n=n)
        assert A.all_ok(res_v) and A.all_ok(res_s)
        assert all(np.array_equal(A.bits(got_v[k]), A.bits(got_s[k])) for k in ("w", "m", "v", "p", "s"))


def test_ema_bound_holds_for_the_fp32_line():
    c = [c for c in A.a_cases() if not c.sparse and c.opt and c.k == 3][0]
    res, got = _run_case(c)
    before, gf = A.case_inputs(c)
    ref = A.case_reference(c, before, before["g"], gf, _factor(c))
    d = F32(0.95)
    s = np.random.default_rng(1).standard_normal(c.n).astype(np.float32)
    s1 = d * s + (F32(1) - d) * got["w"]
    want, bound = A.ema_bound(s, ref.w, ref.bw, float(d))
    r = A.compare(s1.astype(np.float32), want, bound)
    assert r.bad == 0 and r.worst > 0
    assert A.compare((d * s + (F32(1) - d) * before["w"]).astype(np.float32), want, bound).bad > 0        # the weight before the step


# ------------------------------------------------------------------------------------------------------- the free run
@pytest.mark.parametrize("sparse", [False, True])
def test_standin_free_run_stays_inside_the_recurrence(sparse):
    h = A.hyper(A.LR, eps=1e-15 if sparse else 1e-8, wd=A.WD)
    gf = float(F32(1.0) / F32(A.FREE_LOSS_SCALE))
    w0 = (np.random.default_rng(9).standard_normal(A.FREE_N) * 0.1).astype(np.float32)
    run = A.FreeRun(w0, sparse, h, gf)
    with np.errstate(over="ignore"):
        st = dict(w=w0, m=np.zeros_like(w0), v=np.zeros_like(w0), p=w0.astype(np.float16), s=np.zeros(A.FREE_N, np.uint32))
    for t in range(1, A.FREE_STEPS + 1):
        raw, f = A.free_run_gradient(t), float(F32(A.factor64(t, **A.SCHED)))
        st = A.standin_step(st, raw, gf, h, sparse=sparse, zero=True, f32_factor=f, t=t)
        ref = run.step(raw, f)
        if t in A.FREE_RECORD:
            res = {k: A.compare(st[k], getattr(ref, k), getattr(ref, "b" + k)) for k in ("w", "m", "v")}
            print(A.line(f"stand-in free run {'sparse' if sparse else 'dense'} step {t}", res))
            assert A.all_ok(res)
            if sparse:
                assert np.array_equal(st["s"].astype(np.int64), ref.steps)
    assert sparse is False or (ref.steps[15] <= 101 and ref.steps[0] == A.FREE_STEPS and 0 < ref.steps[2] < 120)


# ------------------------------------------------------------------------------------------------------- seeded defects
def _pick(**kw):
    return [c for c in A.a_cases() if all(getattr(c, k) == v for k, v in kw.items())]


WHERE = {
    "bias_correction_at_t_minus_1": lambda: _pick(k=1, half=False, zero=False),
    "g_not_squared": lambda: _pick(k=0, half=False, zero=False),
    "eps_inside_sqrt": lambda: _pick(k=0, half=False, zero=False),
    "coupled_decay": lambda: _pick(k=0, opt=True, zero=False),
    "decay_with_corrected_rate": lambda: _pick(k=0, opt=True, zero=False),
    "betas_swapped_in_rate": lambda: _pick(k=1, half=False, zero=False),
    "inv_loss_scale_twice": lambda: _pick(k=1, zero=False),
    "sparse_decays_skipped_moments": lambda: _pick(sparse=True, k=0),
    "sparse_global_count": lambda: _pick(sparse=True, k=0),
    "quad_skipped_on_first_zero": lambda: _pick(sparse=True, k=0),
    "second_trip_dropped": lambda: [A.size_case(False, False), A.size_case(True, False)],
    "tail_starts_one_late": lambda: _pick(sparse=False, k=0),
    "sparse_rate_off_1e-4": lambda: _pick(sparse=True, k=0),
}


@pytest.mark.parametrize("defect", A.DEFECTS)
def test_seeded_defect_fails_the_gpu_assertions(defect):
    """every case the defect is seeded into must fail, under the assertions test_gpu_adam_float64.py makes (check_step)"""
    cases = WHERE[defect]()
    assert cases
    for c in cases:
        if defect == "second_trip_dropped":
            n = A.SPARSE_BIG if c.sparse else A.DENSE_BIG
            res, _ = _run_case(c, defect=defect, n=n, raw=A.big_sparse_gradient(c.half, c.seed) if c.sparse else None)
        else:
            res, _ = _run_case(c, defect=defect)
        assert not A.all_ok(res), (defect, c)


def test_every_defect_has_its_case():
    assert set(WHERE) == set(A.DEFECTS) and len(A.DEFECTS) == 13
