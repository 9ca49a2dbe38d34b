"""tests/_compositor_float64.py on the CPU: the numpy float64 reference of the training compositors against float64 torch autograd
(an independent derivation), against the C oracle and against a closed form; the fp32 restatements of both schedules inside the
derived bound on the whole ray ladder; every planted defect outside it, with the ladder rays that catch it named, and what a batch
drawn the way the existing tests draw theirs (num_hits <= 12) catches of them; and the bound within the flat bar of the existing
float64 tests on their own inputs.  No GPU.

What the old shapes miss (the gap tests/test_gpu_compositor_float64.py closes), as measured here: in the pair schedule -- the
default training kernel's -- a carry dropped at a 512-sample STEP boundary (P_carry, T_carry) and `cur` not refreshed from `nxt`
pass unnoticed at K = 32 and K = 2; the one-ray schedule's step carries pass at K = 1 (n <= 12) but are caught at K = 7 (n up to
84, two steps), and COMPAT's t carry is caught at K = 32 (six steps at 384 samples).  P_carry dropped at a sub-block boundary,
pincl0 = pincl1, inclusive transmittance, a mask one pair short and S without the background term are caught by the old shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _compositor_float64 as cf                                   # noqa: E402

COLOR = (0.9, 0.25, 1.0)
SCHEDULES = [(32, "pair"), (2, "pair"), (6, "pair"), (130, "pair"), (1, "one"), (7, "one"), (32, "one")]


def _inputs(b, seed=0, background=True):
    """fp16 pixel gradients N(0, 1), a constant background and fp16 alpha gradients for every ray of the batch"""
    rng = np.random.default_rng(seed + b.K)
    g = rng.standard_normal((b.B, 3)).astype(np.float16).astype(np.float64)
    if not background:
        return g, None, None
    bg = np.tile(np.array(COLOR, np.float32), (b.B, 1))
    gA = (0.3 * rng.standard_normal(b.B)).astype(np.float16).astype(np.float64)
    return g, bg, gA


# ---- 1. the reference itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sorted(cf.LADDER))
def test_reference_against_float64_autograd(K):
    """sum_r (pixel_r . g_r + A_r gA_r) differentiated by torch in float64: the formulas of volrender.hip's and
    composite_train.hip's headers are the gradient of the forward, background and alpha term included.  Both sides are float64:
    the distance is held to 1e-12 of the sizes the sums have (mag)."""
    import torch
    b = cf.ladder(K)
    g, bg, gA = _inputs(b)
    ref = cf.gradients(b, g, "pair" if K % 2 == 0 else "one", bg=bg, gA=gA)
    c = torch.from_numpy(b.rad.astype(np.float64)).requires_grad_(True)
    total = torch.zeros((), dtype=torch.float64)
    pix = np.zeros((b.B, 3))
    for r, s in enumerate(cf.ray_slices(b)):                      # per ray: no prefix of one ray leaks rounding into the next
        if s.stop == s.start:
            pix[r] = bg[r]
            continue
        x = torch.from_numpy(b.step[s].astype(np.float64)) * c[s, 3]
        tau = torch.cumsum(x, 0) - x
        w = torch.exp(-tau) * (1 - torch.exp(-x))
        col, A = (w[:, None] * c[s, :3]).sum(0), w.sum()
        p = col + (1 - A) * torch.from_numpy(bg[r].astype(np.float64))
        pix[r] = p.detach().numpy()
        total = total + (p * torch.from_numpy(g[r])).sum() + A * float(gA[r])
    total.backward()
    want = c.grad.numpy()
    assert np.all(np.abs(ref.ref - want) <= 1e-12 * ref.mag + 1e-300), np.abs(ref.ref - want).max()
    np.testing.assert_allclose(ref.pix, pix, rtol=0, atol=1e-13)
    assert np.abs(want[:, 3]).max() > 1e-2 and np.abs(want[:, :3]).max() > 1e-2


@pytest.mark.parametrize("K", [32, 7, 1])
def test_reference_against_the_c_oracle(oracle, K):
    """volrender_fwd_nerf and volrender_bwd_nerf evaluate in double and store float32: within one float32 rounding of the
    reference (u |ref|, and 1e-12 of the sums' sizes for the order of the double sums).  volrender_bwd (COMPAT) is float32
    rounded to fp16: within one fp16 ulp of half(float64), as the kernel is asked to be.  l2_loss: values float32, gradients
    fp16 of loss_scale 2 e / N."""
    b = cf.ladder(K)
    g, _, _ = _inputs(b, background=False)
    ref = cf.gradients(b, g, "one")
    pix = oracle.volrender_fwd_nerf(b.rad, b.nh, b.idx, b.step, K=K).astype(np.float64)
    assert np.all(np.abs(pix - ref.pix) <= cf.U * np.abs(ref.pix) + 1e-12)
    got = oracle.volrender_bwd_nerf(g.astype(np.float16), b.rad, b.step, b.nh, b.idx, K=K).astype(np.float64)
    assert np.all(np.abs(got - ref.ref) <= cf.U * np.abs(ref.ref) + 1e-12 * ref.mag + 2.0 ** -150)
    for t in (b.t_regular, b.t_jitter):
        compat = oracle.volrender_bwd(g.astype(np.float16), b.rad, t, b.nh, b.idx, K=K)
        assert cf.compat_ulps(compat, cf.compat_backward(b, g, t)).max() <= 1
    tgt = b.tgt[:, :3]
    p32 = ref.pix.astype(np.float32)
    total, values, g16, _ = oracle.l2_loss(p32, tgt, scale=128.0)
    e = p32.astype(np.float64) - tgt.astype(np.float64)
    l, dl = cf.loss_terms("l2", e, None, None)
    np.testing.assert_allclose(values.reshape(-1, 3), l / (3 * b.B), rtol=4 * cf.U, atol=1e-30)
    assert abs(total - l.sum() / (3 * b.B)) <= 1e-6 * total
    assert np.abs(cf.half_order(g16.reshape(-1, 3)) - cf.half_order((128.0 * dl / (3 * b.B)).astype(np.float16))).max() <= 1


def test_reference_closed_form_constant_density():
    """One ray of constant density and colour (test_aux_closed_form_constant_density's form): w_i = q^i (1 - q), q = exp(-x), so
    A = 1 - q^n, pixel = c A + (1 - A) b, and with G = g.c - g.b + g_A the same for every sample
    dL/dsigma_i = d G q^n (T_i e^{-x} G - G (T_{i+1} - q^n) telescopes to that)."""
    for sigma, step, n in ((3.0, 0.05, 32), (20.0, 0.01, 64), (0.5, 0.02, 640)):
        rad = np.zeros((n, 4), np.float32)
        rad[:, :3], rad[:, 3] = 0.5, sigma
        d = np.full(n, step, np.float32)
        b = cf.as_batch(1, [n], rad, d, np.zeros((1, 4), np.float32))
        g, bgc, gA = np.array([[0.5, -0.25, 1.0]]), np.array([COLOR], np.float32), np.array([0.125])
        ref = cf.gradients(b, g, "one", bg=bgc, gA=gA)
        q = np.exp(-float(d[0]) * sigma)
        A = 1 - q ** n
        G = float(g[0] @ rad[0, :3] - g[0] @ bgc[0].astype(np.float64) + gA[0])
        assert abs(ref.A[0] - A) < 1e-13
        np.testing.assert_allclose(ref.pix[0], 0.5 * A + (1 - A) * bgc[0].astype(np.float64), rtol=0, atol=1e-13)
        np.testing.assert_allclose(ref.ref[:, 3], float(d[0]) * G * q ** n, rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(ref.ref[:, 0], g[0, 0] * q ** np.arange(n) * (1 - q), rtol=1e-12, atol=0)


def test_distortion_gradient_is_the_pairwise_sums_gradient():
    """q of distortion_pairwise against float64 autograd of the pairwise double sum it states"""
    import torch
    rng = np.random.default_rng(4)
    n = 700
    w, m, width = rng.uniform(0, 0.01, n), np.sort(rng.uniform(0.1, 6.0, n)), rng.uniform(0.001, 0.05, n)
    L, q = cf.distortion_pairwise(w, m, width)
    wt, mt = torch.from_numpy(w).requires_grad_(True), torch.from_numpy(m)
    Lt = (wt[:, None] * wt[None, :] * (mt[:, None] - mt[None, :]).abs()).sum() + (wt * wt * torch.from_numpy(width)).sum() / 3.0
    qt, = torch.autograd.grad(Lt, wt)
    assert abs(L - float(Lt.detach())) <= 1e-12 * L
    np.testing.assert_allclose(q, qt.numpy(), rtol=1e-11, atol=0)


# ---- 2. a faithful kernel stays inside the bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K,schedule", SCHEDULES)
@pytest.mark.parametrize("background", [False, True])
def test_fp32_restatement_stays_inside_the_bound(K, schedule, background):
    """the whole ladder, every regime, both ways of forming S; no element left out (the restatement's NaN pre-fill would fail)"""
    b = cf.ladder(K)
    g, bg, gA = _inputs(b, background=background)
    ref = cf.gradients(b, g, schedule, bg=bg, gA=gA)
    for S_from in ("pixel",) if background else ("pixel", "sum"):
        got = cf.emulate(b, g, schedule, bg=bg, gA=gA, S_from=S_from)
        table = cf.check_elements(f"K={K} {schedule} S from {S_from}", got, ref.ref, ref.bound, b)
        for line in cf.table_lines(f"restatement K={K} {schedule} bg={background} S={S_from}", table):
            print(line)
        assert set(table) == set(cf.REGIMES)


@pytest.mark.parametrize("K,schedule", [(32, "pair"), (2, "pair"), (7, "one")])
def test_fp32_restatement_with_the_regulariser_stays_inside_the_bound(K, schedule):
    """composite_train_*<true>: k = loss_scale lambda_d / n_rays with loss scale 128 and lambda_d = 1; without the term the same
    restatement is far outside the bound, so the bound sees the regulariser"""
    b = cf.ladder(K)
    g, bg, gA = _inputs(b)
    k = float(np.float32(128.0) * np.float32(1.0) / np.float32(b.B))
    ref = cf.gradients(b, g, schedule, bg=bg, gA=gA, reg_k=k)
    table = cf.check_elements(f"K={K} {schedule} REG", cf.emulate(b, g, schedule, bg=bg, gA=gA, reg_k=k), ref.ref, ref.bound, b)
    for line in cf.table_lines(f"restatement K={K} {schedule} REG", table):
        print(line)
    assert cf.failing_rays(cf.emulate(b, g, schedule, bg=bg, gA=gA), ref.ref, ref.bound, b)


@pytest.mark.parametrize("K", [32, 7, 1])
def test_fp32_compat_restatement_is_within_one_ulp(K):
    b = cf.ladder(K)
    g, _, _ = _inputs(b, background=False)
    for t in (b.t_regular, b.t_jitter):
        assert cf.compat_ulps(cf.emulate_compat(b, g, t), cf.compat_backward(b, g, t)).max() <= 1


# ---- 3. planted defects fall outside it ----------------------------------------------------------------------------------------------
# (K, schedule, defect): ladder rays that must be among those that catch it.  impulse_before puts all of a ray's weight into the
# last sample before the last multiple of 64, i.e. right before a lane-32, sub-block or step boundary.
CATCHERS = {
    (32, "pair", "P_carry_step"): ["impulse_before n=544", "impulse_before n=1056", "sparse n=4096"],
    (32, "pair", "P_carry_block"): ["impulse_before n=160", "impulse_before n=544", "sparse n=256"],
    (32, "pair", "T_carry_step"): ["impulse_before n=544", "impulse_before n=1056", "sparse n=4096"],
    (32, "pair", "pincl0_is_pincl1"): ["impulse_before n=96", "impulse_before n=4096", "benign n=32"],
    (32, "pair", "inclusive_T"): ["impulse n=32", "impulse n=4096", "benign n=32"],
    (32, "pair", "stale_cur"): ["transparent n=544", "transparent n=4096", "impulse n=1056", "impulse_before n=1024"],
    (32, "pair", "short_mask"): ["transparent n=32", "benign n=4096", "impulse n=544"],
    (32, "pair", "S_without_bg"): ["impulse n=32", "sparse n=4096", "benign n=512"],
    (2, "pair", "P_carry_step"): ["impulse_before n=514", "impulse_before n=1026"],
    (2, "pair", "P_carry_block"): ["impulse_before n=130", "impulse_before n=258", "impulse_before n=514"],
    (2, "pair", "T_carry_step"): ["impulse_before n=514", "impulse_before n=1026"],
    (2, "pair", "pincl0_is_pincl1"): ["impulse_before n=66", "impulse_before n=1024"],
    (2, "pair", "inclusive_T"): ["impulse n=2", "impulse n=1026"],
    (2, "pair", "stale_cur"): ["transparent n=514", "transparent n=1022", "impulse n=1026"],
    (2, "pair", "short_mask"): ["transparent n=2", "transparent n=510", "transparent n=1026"],
    (2, "pair", "S_without_bg"): ["impulse n=2", "impulse n=1026"],
    (7, "one", "P_carry_step"): ["impulse_before n=70", "impulse_before n=518"],
    (7, "one", "T_carry_step"): ["impulse_before n=70", "impulse_before n=518"],
    (7, "one", "inclusive_T"): ["impulse n=7", "impulse n=518"],
    (7, "one", "short_mask"): ["transparent n=7", "transparent n=63", "transparent n=518"],
    (7, "one", "S_without_bg"): ["impulse n=7", "impulse n=518"],
    (1, "one", "P_carry_step"): ["impulse_before n=65", "impulse_before n=129", "impulse_before n=193"],
    (1, "one", "T_carry_step"): ["impulse_before n=65", "impulse_before n=129", "impulse_before n=193"],
    (1, "one", "inclusive_T"): ["impulse n=1", "impulse n=193"],
    (1, "one", "short_mask"): ["transparent n=1", "transparent n=64", "transparent n=193"],
    (1, "one", "S_without_bg"): ["impulse n=1", "impulse n=193"],
}
# what a batch of the old shapes (num_hits <= 12, benign samples, 777 rays) catches: True = some ray falls outside the bound
OLD_SHAPES_CATCH = {
    (32, "pair"): dict(P_carry_step=False, P_carry_block=True, T_carry_step=False, pincl0_is_pincl1=True, inclusive_T=True,
                       stale_cur=False, short_mask=True, S_without_bg=True),
    (2, "pair"): dict(P_carry_step=False, P_carry_block=False, T_carry_step=False, pincl0_is_pincl1=True, inclusive_T=True,
                      stale_cur=False, short_mask=True, S_without_bg=True),
    (7, "one"): dict(P_carry_step=True, T_carry_step=True, inclusive_T=True, short_mask=True, S_without_bg=True),
    (1, "one"): dict(P_carry_step=False, T_carry_step=False, inclusive_T=True, short_mask=True, S_without_bg=True),
}


@pytest.mark.parametrize("K,schedule", sorted(OLD_SHAPES_CATCH))
def test_planted_defects_fall_outside_the_bound(K, schedule):
    b, old = cf.ladder(K), cf.old_shapes(K)
    g, bg, gA = _inputs(b)
    ref = cf.gradients(b, g, schedule, bg=bg, gA=gA)
    go, bgo, gAo = _inputs(old, seed=9)
    ref_old = cf.gradients(old, go, schedule, bg=bgo, gA=gAo)
    assert not cf.failing_rays(cf.emulate(old, go, schedule, bg=bgo, gA=gAo), ref_old.ref, ref_old.bound, old)
    for defect in cf.DEFECTS_PAIR if schedule == "pair" else cf.DEFECTS_ONE:
        caught = cf.failing_rays(cf.emulate(b, g, schedule, bg=bg, gA=gA, defect=defect), ref.ref, ref.bound, b)
        missing = [x for x in CATCHERS[(K, schedule, defect)] if x not in caught]
        print(f"defect {defect} K={K} {schedule}: caught by {len(caught)} ladder rays, among them {CATCHERS[(K, schedule, defect)]}")
        assert not missing, (defect, missing, caught)
        by_old = cf.failing_rays(cf.emulate(old, go, schedule, bg=bgo, gA=gAo, defect=defect), ref_old.ref, ref_old.bound, old)
        print(f"    old shapes (num_hits <= 12): {'caught by ' + ', '.join(by_old[:4]) if by_old else 'missed'}")
        assert bool(by_old) == OLD_SHAPES_CATCH[(K, schedule)][defect], (defect, by_old)


@pytest.mark.parametrize("K", [32, 7, 1])
def test_compat_carry_reset_at_a_step_is_more_than_one_ulp(K):
    """t_carry reset to 0 at a 64-sample step: the first sample of every later step takes delta = t instead of t - t_prev.
    Caught on the ladder by every ray above 64 samples with a non-zero density there; the old shapes catch it too at K = 32 and
    K = 7 (384 and 84 samples are six and two steps) and miss it at K = 1 (12 samples)."""
    b, old = cf.ladder(K), cf.old_shapes(K)
    g, _, _ = _inputs(b, background=False)
    go, _, _ = _inputs(old, seed=9, background=False)
    for name in ("t_regular", "t_jitter"):
        t = getattr(b, name)
        ulps = cf.compat_ulps(cf.emulate_compat(b, g, t, defect="t_carry_step"), cf.compat_backward(b, g, t))
        rays = sorted({cf.label(b, r) for r, s in enumerate(cf.ray_slices(b)) if (ulps[s] > 1).any()})
        print(f"COMPAT t_carry reset, K={K} {name}: {int((ulps > 1).sum())} elements above one ulp, rays {rays[:6]}")
        assert f"dense n={max(cf.LADDER[K]) * K}" in rays and f"benign n={max(cf.LADDER[K]) * K}" in rays
        to = getattr(old, name)
        ulps_old = cf.compat_ulps(cf.emulate_compat(old, go, to, defect="t_carry_step"), cf.compat_backward(old, go, to))
        assert bool((ulps_old > 1).any()) == (K != 1)


# ---- 4. the bound against the existing flat bar -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("case", ["none3", "constant4", "random4"])
def test_bound_is_within_the_flat_bar_on_the_existing_inputs(case, K):
    """case_inputs of tests/test_gpu_train_loss.py (777 rays, loss scale 128, L2 and lambda = 0.5 where the targets are RGBA), g and
    g_A formed from the float64 pixels: no element's bound exceeds 1.5e-3 |ref| + 2e-5."""
    import test_gpu_train_loss as tl
    nh, idx, P, rad, step, tgt, bg_np = tl.case_inputs(K, case)
    b = cf.as_batch(K, nh, rad, step, tgt)
    assert np.array_equal(b.idx, idx)
    zero = np.zeros((b.B, 3))
    fwd = cf.gradients(b, zero, "pair" if K % 2 == 0 else "one", bg=bg_np)
    e = fwd.pix - cf.composited_target(bg_np, tgt)
    g = (tl.LS * 2 * e / (3 * b.B)).astype(np.float16).astype(np.float64)
    lam = 0.0 if case == "none3" else tl.LAMBDA
    gA = None if case == "none3" else (tl.LS * lam * 2 * (fwd.A - tgt[:, 3].astype(np.float64)) / b.B).astype(np.float16).astype(np.float64)
    ref = cf.gradients(b, g, "pair" if K % 2 == 0 else "one", bg=None if case == "none3" else bg_np, gA=gA)
    flat = 1.5e-3 * np.abs(ref.ref) + 2e-5
    share = ref.bound / flat
    print(f"[{case} K={K}] bound / flat bar: max {share.max():.3f}, median {np.median(share):.3f}")
    assert np.all(ref.bound <= flat)
    assert np.abs(ref.ref[:, 3]).max() > 1e-3
