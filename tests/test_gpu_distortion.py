"""The distortion regulariser on the GPU (include/rtxn.h, rtxn_train_regularizer): the regularised compositor
(composite_train.hip, REG = true) against float64 autograd of the pairwise double sum; weight 0 is the existing call bit for bit; the
traversal's t_start / t_end as the trainer plumbs them; agreement of the eager / captured / one-call steps; the fixed-order loss
sum of deterministic mode; and end-to-end training on the sphere teacher.

Measured values: profiles/r10/distortion_tests.txt."""
import faulthandler
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _compositor_float64 import distortion_pairwise      # noqa: E402  (the pairwise double sum and its gradient, float64)

B_RAYS, LS = 777, 128.0
LAMBDA_D = 10.0                                         # with loss scale 128: the term is of the colour term's size
LAMBDA_A = 0.5
DELTA = np.float32(0.1)                                 # api.train_loss("huber")'s default
COLOR = (0.9, 0.25, 1.0)
SEED = 1026
# (loss kind, background case): L2 without a background, Huber over a constant background with RGBA targets and the alpha term
CASES = {"l2_none3": ("l2", None, 0.0), "huber_constant4": ("huber", COLOR, LAMBDA_A)}


@pytest.fixture(autouse=True)
def _own_timeout():
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _to_dev(torch, **arrays):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}


_CASES = {}


def case_inputs(K, case, t_scale=1.0):
    """t_scale != 1: the batch as a trainer with that density_scale hands it over -- the compositor's step lengths multiplied by
    it and sigma divided by it (rtxn_train_batch.t_scale), the distances untouched.  One (K, case), made once and never changed; no GPU involved.  The batch shapes of tests/test_gpu_train_loss.py: every 7th
    ray empty, a few rays above 512 samples.  Segments of a ray are ascending and disjoint: every second gap is 0 (cells that
    touch, as the grid walk leaves them), the others up to 0.3; a segment's step is uniform in (0.01, 0.2) as that test's steps
    are, its length K steps, and step = (t_end - t_start) / K in fp32 is what the compositor reads."""
    key = (K, case, t_scale)
    if t_scale != 1.0 and key not in _CASES:
        nh, idx, P, rad, step, ts, te, tgt, bg_np = case_inputs(K, case)
        rad = rad.copy()
        rad[:, 3] /= np.float32(t_scale)
        _CASES[key] = (nh, idx, P, rad, step * np.float32(t_scale), ts, te, tgt, bg_np)
    if key not in _CASES:
        rng = np.random.default_rng(K * 7 + len(case) + SEED)
        B = B_RAYS
        nh = rng.integers(0, 8, B).astype(np.int32)
        nh[::7] = 0
        nh[3::50] = rng.integers(17, 40, nh[3::50].size)
        idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
        P = int(nh.sum())
        rad = np.concatenate([rng.uniform(0, 1, (P * K, 3)), rng.uniform(0, 1.5, (P * K, 1))], 1).astype(np.float32)
        length = (rng.uniform(0.01, 0.2, P) * K).astype(np.float32)
        gap = (rng.uniform(0.0, 0.3, P) * rng.integers(0, 2, P)).astype(np.float32)
        first = rng.uniform(0.1, 1.0, B).astype(np.float32)
        ts, te = np.zeros(P, np.float32), np.zeros(P, np.float32)
        for r in range(B):
            t = first[r]
            for j in range(idx[r], idx[r] + nh[r]):
                ts[j] = t
                te[j] = np.float32(t + length[j])
                t = np.float32(te[j] + gap[j])
        assert np.all(te > ts)
        step = np.repeat((te - ts) / np.float32(K), K)
        assert step.dtype == np.float32
        kind, color, lam = CASES[case]
        tc = 3 if color is None else 4
        tgt = rng.uniform(0, 1, (B, tc)).astype(np.float32)
        if tc == 4:
            tgt[::5, 3] = 0.0
            tgt[1::5, 3] = 1.0
        bg_np = np.zeros((B, 3), np.float32) if color is None else np.tile(np.array(color, np.float32), (B, 1))
        _CASES[key] = (nh, idx, P, rad, step, ts, te, tgt, bg_np)
    return _CASES[key]


def _composited(bg, tgt):
    """the target the kernel fits: RGBA composited over the background in fp32, as include/rtxn.h defines it"""
    if tgt.shape[1] == 3:
        return tgt.astype(np.float64)
    a = tgt[:, 3:4]
    t = a * tgt[:, :3] + (np.float32(1.0) - a) * bg
    assert t.dtype == np.float32
    return t.astype(np.float64)


def loss_terms(kind, e):
    """float64: l(e) and dl/dp of include/rtxn.h's table"""
    if kind == "l2":
        return e * e, 2 * e
    delta = float(DELTA)
    a = np.abs(e)
    return np.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta)), np.clip(e, -delta, delta)


_REFS = {}


def reference(torch, K, case, t_scale=1.0):
    """float64, made once per (K, case, t_scale): c (radiance with autograd), w, pixels, A, depth = sum w m, L_r = the PAIRWISE
    double sum sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i with delta_i = (t_end - t_start) / K as include/rtxn.h
    defines it (the compositor's step length where t_scale = 1, to an ulp), and q = dL_r/dw of that sum -- both stated once, in
    tests/_compositor_float64.py (distortion_pairwise; tests/test_compositor_float64_reference.py holds its q to autograd)."""
    key = (K, case, t_scale)
    if key not in _REFS:
        nh, idx, P, rad, step, ts, te, tgt, bg_np = case_inputs(K, case, t_scale)
        B = nh.shape[0]
        ray = torch.from_numpy(np.repeat(np.arange(B), nh * K))
        c = torch.from_numpy(rad.astype(np.float64)).requires_grad_(True)
        d = torch.from_numpy(step.astype(np.float64))
        x = d * c[:, 3]
        cs = torch.cumsum(x, 0)
        start = np.concatenate([[0], np.cumsum(nh * K)[:-1]])
        off = torch.cat([torch.zeros(1, dtype=torch.float64), cs])[torch.from_numpy(start)][ray]
        w = torch.exp(-(cs - x - off)) * (1 - torch.exp(-x))
        col = torch.zeros((B, 3), dtype=torch.float64).index_add(0, ray, w[:, None] * c[:, :3])
        A = torch.zeros(B, dtype=torch.float64).index_add(0, ray, w)
        pix = col + (1 - A)[:, None] * torch.from_numpy(bg_np.astype(np.float64))
        k = np.tile(np.arange(K, dtype=np.float64), P)
        ts64, te64 = np.repeat(ts.astype(np.float64), K), np.repeat(te.astype(np.float64), K)
        m = torch.from_numpy(ts64 + (k + 0.5) / K * (te64 - ts64))
        width = torch.from_numpy((te64 - ts64) / K)
        depth = torch.zeros(B, dtype=torch.float64).index_add(0, ray, w.detach() * m)
        L = np.zeros(B)
        q = torch.zeros_like(m)
        w_np, m_np, width_np = w.detach().numpy(), m.numpy(), width.numpy()
        for r in range(B):
            if nh[r] == 0:
                continue
            s = slice(int(start[r]), int(start[r]) + int(nh[r]) * K)
            L[r], q_r = distortion_pairwise(w_np[s], m_np[s], width_np[s])
            q[s] = torch.from_numpy(q_r)
        _REFS[key] = (c, w, pix, A, depth.numpy(), L, q, m.numpy())
    return _REFS[key]


def _structs(torch, api, case, weight, B, P, dev, outputs=True, opacity=True):
    kind, color, lam = CASES[case]
    bg = None if color is None else api.train_background(color, target_channels=4)
    opa = torch.full((B,), -1.0, device="cuda") if opacity else None
    spec = api.train_loss(kind, opacity_weight=lam, opacity=opa)
    dist = torch.full((B,), -1.0, device="cuda") if outputs else None
    dep = torch.full((B,), -1.0, device="cuda") if outputs else None
    reg = api.train_regularizer(weight, dev["ts"], dev["te"], dist, dep)
    return bg, spec, reg, opa, dist, dep


def _run(torch, api, K, case, weight=LAMBDA_D, t_scale=1.0, misaligned=False, **kw):
    """misaligned: the step lengths are handed over as a view that starts 4 bytes into its allocation"""
    nh, idx, P, rad, step, ts, te, tgt, bg_np = case_inputs(K, case, t_scale)
    B = B_RAYS
    dev = _to_dev(torch, rad=rad, step=step, nh=nh, idx=idx, tgt=tgt, ts=ts, te=te)
    if misaligned:
        dev["step"] = torch.cat([torch.zeros(1, device="cuda"), dev["step"]])[1:]
        assert dev["step"].data_ptr() % 8 == 4 and dev["step"].is_contiguous()
    bg, spec, reg, opa, dist, dep = _structs(torch, api, case, weight, B, P, dev, **kw)
    pix = torch.zeros((B, 3), device="cuda")
    lg = torch.zeros((B, 3), dtype=torch.float16, device="cuda")
    loss = torch.full((1,), 9.0, device="cuda")           # a stale value: the call must replace it
    out = torch.zeros((P * K, 4), dtype=torch.float16, device="cuda")
    api.volrender_reg_train(dev["rad"], dev["step"], dev["nh"], dev["idx"], B, K, dev["tgt"], LS, pix, lg, loss, out, bg, spec, reg)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in
            dict(pix=pix, lg=lg, loss=loss, out=out, opa=opa, dist=dist, dep=dep).items()}


# ---- 1. the compositor against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("case", list(CASES))
def test_reg_compositor_against_float64_autograd(gpu, case, K):
    """K = 32: composite_train_multi_kernel<true, 4>; K = 7: composite_train_kernel<true>.  lambda_d = 10, loss scale 128.  Pixels and A keep the
    loss test's bars; depth within 3e-6 max(m) of sum w m (max over the ray's own samples, which asks no less than the batch's);
    L_r within 2e-5 of the largest L_r; the loss scalar within 1e-5 relative; radiance gradients rtol 1.5e-3, atol 2e-5 against
    autograd of pixels.g + A.g_A + k sum_r L_r (g, g_A: the kernel's own fp16 values; k = loss_scale lambda_d / n_rays in fp32).
    The distortion part of the wanted sigma-gradient alone exceeds 1e-3 and moves at least half of the non-zero sigma-gradients
    by more than their bar: without the term the test cannot pass."""
    _check_compositor(gpu, case, K, 1.0)


def _check_compositor(torch, case, K, t_scale, misaligned=False, results=None):
    from rtx_nerf_amd import api
    nh, idx, P, rad, step, ts, te, tgt, bg_np = case_inputs(K, case, t_scale)
    kind, color, lam = CASES[case]
    B = B_RAYS
    got = _run(torch, api, K, case, t_scale=t_scale, misaligned=misaligned)
    if results is not None:
        results.append(got)
    c, w, ref_pix_t, ref_A_t, ref_depth, ref_L, q, m = reference(torch, K, case, t_scale)
    ref_pix, ref_A = ref_pix_t.detach().numpy(), ref_A_t.detach().numpy()
    e = ref_pix - _composited(bg_np, tgt)
    l, _ = loss_terms(kind, e)
    alpha = tgt[:, 3].astype(np.float64) if tgt.shape[1] == 4 else np.zeros(B)
    ref_loss = float(l.sum() / (3 * B) + float(np.float32(lam)) / B * ((ref_A - alpha) ** 2).sum() + LAMBDA_D / B * ref_L.sum())
    loss_err = abs(float(got["loss"][0]) - ref_loss) / ref_loss
    pix_err, A_err = np.abs(got["pix"] - ref_pix).max(), np.abs(got["opa"] - ref_A).max()
    starts = np.concatenate([[0], np.cumsum(nh * K)])
    m_max = np.array([m[starts[r]:starts[r + 1]].max() if nh[r] else 0.0 for r in range(B)])
    depth_ratio = (np.abs(got["dep"] - ref_depth)[nh > 0] / (3e-6 * m_max[nh > 0])).max()
    L_err = np.abs(got["dist"] - ref_L).max() / ref_L.max()
    # radiance gradients: g_A recomputed from the kernel's own A by the kernel's operations (fp32, then fp16)
    inv_rays = np.float32(1.0) / np.float32(B)
    gA = (np.float32(LS) * (np.float32(lam) * (np.float32(2.0) * (got["opa"] - alpha.astype(np.float32)))) * inv_rays).astype(np.float16)
    k = float(np.float32(LS) * np.float32(LAMBDA_D) / np.float32(B))
    if c.grad is not None:
        c.grad = None
    w.backward(k * q, retain_graph=True)
    dist_part = c.grad.numpy().copy()
    ((ref_pix_t * torch.from_numpy(got["lg"].astype(np.float64))).sum()
     + (ref_A_t * torch.from_numpy(gA.astype(np.float64))).sum()).backward(retain_graph=True)
    want = c.grad.numpy().copy()
    have = got["out"].astype(np.float64)
    # sigma is the batch's, 1 / t_scale of the world's: its gradient is t_scale times the world's, and so is its absolute bar
    atol = np.array([2e-5, 2e-5, 2e-5, 2e-5 * t_scale])
    bar = 1.5e-3 * np.abs(want) + atol
    ratio = np.abs(have - want) / bar
    nz = want[:, 3] != 0.0
    moved = (np.abs(dist_part[:, 3]) > bar[:, 3])[nz].mean()
    print(f"\n[{case} K={K} t_scale={t_scale}{' misaligned' if misaligned else ''}] pixels max|err| {pix_err:.2e}  opacity max|err| {A_err:.2e}  depth max err / (3e-6 max m) {depth_ratio:.3f}  "
          f"L_r max|err| / max L_r {L_err:.2e} (max L_r {ref_L.max():.3f})  loss {ref_loss:.5f} (distortion part "
          f"{LAMBDA_D / B * ref_L.sum():.5f}) rel {loss_err:.2e}  radiance grads max|err| {np.abs(have - want).max():.2e}, "
          f"max err / (1.5e-3 |want| + 2e-5) {ratio.max():.3f}  distortion part of the sigma-gradient: max {np.abs(dist_part[:, 3]).max():.3e}, "
          f"moves {moved:.3f} of the non-zero sigma-gradients by more than the bar")
    empty = nh == 0
    assert np.array_equal(got["pix"][empty], bg_np[empty]) and np.all(got["opa"][empty] == 0.0)
    assert np.all(got["dist"][empty] == 0.0) and np.all(got["dep"][empty] == 0.0)
    np.testing.assert_allclose(got["pix"], ref_pix, rtol=0, atol=3e-6)
    np.testing.assert_allclose(got["opa"], ref_A, rtol=0, atol=3e-6)
    assert depth_ratio <= 1.0
    assert L_err <= 2e-5
    assert ref_loss > 1e-3 and loss_err < 1e-5
    assert ratio.max() <= 1.0, ratio.max()
    assert np.abs(dist_part[:, 3]).max() > 1e-3 and np.all(dist_part[:, :3] == 0.0)
    assert moved >= 0.5
    return w.detach().numpy(), step, ref_L, got["dist"]


def test_misaligned_step_lengths_take_the_one_ray_kernel_at_an_even_K(gpu):
    """K = 32 with the step lengths 4 bytes off an 8-byte boundary: the pair schedule reads them two at a time, so the call
    must run composite_train_kernel<true>, the one-ray form, which the other tests reach at an odd K only.  Every bar of
    test_reg_compositor_against_float64_autograd holds for it against the same float64 reference, and its pixels and fp16 loss
    gradients are the aligned call's within the pixels' bar and one fp16 ulp.  Huber over a constant background, RGBA targets,
    the alpha term, lambda_d = 10.  Measured on an MI355X (profiles/r12/compositor_merge_ab.txt): against float64 pixels
    1.90e-7, opacities 2.92e-7, depth 0.060 of its bar, L_r 4.0e-7 of the largest, loss 2.1e-8 relative, radiance gradients
    0.299 of their bar (aligned: the same but L_r 4.4e-7 and loss 2.0e-7); aligned against misaligned pixels within 2.4e-7,
    all 2331 fp16 loss gradients equal.  No bar needed widening."""
    case, K = "huber_constant4", 32
    res = []
    _check_compositor(gpu, case, K, 1.0, results=res)
    _check_compositor(gpu, case, K, 1.0, misaligned=True, results=res)
    a, b = res
    pix_diff = np.abs(a["pix"] - b["pix"]).max()
    ulps = np.abs(_half_order(a["lg"]) - _half_order(b["lg"]))
    print(f"[{case} K={K}] aligned against misaligned: pixels max|diff| {pix_diff:.2e}  fp16 loss gradients: {int((ulps != 0).sum())} of "
          f"{ulps.size} differ, max {int(ulps.max())} ulp")
    np.testing.assert_allclose(a["pix"], b["pix"], rtol=0, atol=3e-6)
    assert ulps.max() <= 1


def _half_order(x):
    """fp16 values as integers ordered like the values: differences are distances in units of the last place"""
    i = x.view(np.int16).astype(np.int32)
    return np.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("case,K", [("huber_constant4", 32), ("l2_none3", 7)])
def test_step_lengths_with_a_density_scale_leave_the_distances_alone(gpu, case, K):
    """The batch of a trainer with density_scale 120: the compositor's step lengths are 120 times the intervals' widths and sigma
    1 / 120 of the world's.  delta_i is the width, from t_start / t_end: every bar of the test above holds against the same
    float64 reference (the sigma-gradient's absolute bar times 120, as the gradient is).  Read from the step lengths instead, the
    self term would be 120 times too large -- far outside L_r's bar, which the test also shows."""
    w, step, ref_L, got_L = _check_compositor(gpu, case, K, 120.0)
    nh = case_inputs(K, case)[0]
    ray = np.repeat(np.arange(B_RAYS), nh * K)
    self_term = np.bincount(ray, weights=w * w * step.astype(np.float64), minlength=B_RAYS) / 3.0      # with the step lengths read
    wrong = ref_L + self_term * (1.0 - 1.0 / 120.0)
    print(f"[{case} K={K}] L_r with delta read from the step lengths: up to {np.abs(wrong - ref_L).max() / ref_L.max():.3f} of max L_r away")
    assert np.abs(wrong - got_L).max() / ref_L.max() > 100 * 2e-5


# ---- 2. weight 0 means no change -----------------------------------------------------------------------------------------------
def test_weight_zero_is_the_existing_call_bit_for_bit(gpu):
    """regularizer None, and weight 0 without outputs (with or without t buffers): bitwise the pixels, fp16 loss gradients,
    opacities and radiance gradients of rtxn_volrender_loss_train; the scalar bitwise where its order is fixed (a deterministic
    workspace registered), and within the float atomics' own bound in default mode (tests/test_gpu_train_loss.py's count)."""
    torch = gpu
    from rtx_nerf_amd import api
    for K in (32, 7):
        for case in CASES:
            nh, idx, P, rad, step, ts, te, tgt, bg_np = case_inputs(K, case)
            B = B_RAYS
            dev = _to_dev(torch, rad=rad, step=step, nh=nh, idx=idx, tgt=tgt, ts=ts, te=te)
            atomics_bar = 2 * (((B + 3) // 4 if K % 2 == 0 else B) + 10) * 2.0 ** -24
            for deterministic in (False, True):
                shadow = api.deterministic_shadow(64) if deterministic else None
                api.set_deterministic(shadow, None)
                try:
                    res = []
                    for form in ("loss", "none", "zero", "zero_t"):
                        bg, spec, _, opa, _, _ = _structs(torch, api, case, 0.0, B, P, dev, outputs=False)
                        pix, lg = torch.zeros((B, 3), device="cuda"), torch.zeros((B, 3), dtype=torch.float16, device="cuda")
                        out = torch.zeros((P * K, 4), dtype=torch.float16, device="cuda")
                        loss = torch.full((1,), 9.0, device="cuda")
                        a = (dev["rad"], dev["step"], dev["nh"], dev["idx"], B, K, dev["tgt"], LS, pix, lg, loss, out, bg, spec)
                        if form == "loss":
                            api.volrender_loss_train(*a)
                        else:
                            api.volrender_reg_train(*a, None if form == "none" else api.train_regularizer(0.0) if form == "zero"
                                                    else api.train_regularizer(0.0, dev["ts"], dev["te"]))
                        torch.cuda.synchronize()
                        res.append((pix, lg, out, opa, float(loss.item())))
                finally:
                    api.set_deterministic(None, None)
                for r in res[1:]:
                    for x, y in zip(res[0][:4], r[:4]):
                        assert torch.equal(x, y), (K, case, deterministic)
                    if deterministic:
                        assert r[4] == res[0][4], (K, case)
                    else:
                        assert abs(r[4] - res[0][4]) <= atomics_bar * abs(res[0][4]), (K, case)
                assert float(res[0][2].float().abs().max()) > 0.0


# ---- 5. deterministic mode ---------------------------------------------------------------------------------------------------
# Huber + alpha over a background, against float64: tests/test_gpu_train_loss.py counts at most 9 roundings on a ray's colour +
# alpha term.  The distortion share weight * L * inv_rays from the stored L_r: two products and the rounded 1 / n_rays, 3; the
# ray's term is their sum, one more rounding on either path: max(9, 3) + 1 = 10; the fixed-order sum adds at most 14 (that
# test's count): 24, and (1 + u)^24 - 1 < 25 u.
DET_BAR = 25 * 2.0 ** -24


def _fixed_order_l2(pix, tgt, dist, weight):
    """rtxn's fixed-order sum restated in fp32, operation for operation, for L2 without a background: per ray
    ((e0^2 + e1^2 + e2^2) * (1 / (3 n))) + (weight * L_r) * (1 / n); groups of four as (a + b) + (c + d); one group per thread of
    1024 (n <= 4096); a halving tree over the threads."""
    f = np.float32
    B = pix.shape[0]
    inv_n, inv_rays = f(1.0) / f(3 * B), f(1.0) / f(B)
    e = pix - tgt
    sq = e * e
    v = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) * inv_n
    v = v + (f(weight) * dist) * inv_rays
    assert v.dtype == np.float32
    g = np.zeros(4 * ((B + 3) // 4), np.float32)
    g[:B] = v
    g = g.reshape(-1, 4)
    red = np.zeros(1024, np.float32)
    red[:g.shape[0]] = (g[:, 0] + g[:, 1]) + (g[:, 2] + g[:, 3])
    n = 512
    while n:
        red[:n] = red[:n] + red[n:2 * n]
        n //= 2
    return red[0]


@pytest.mark.parametrize("K", [32, 7])
def test_deterministic_loss_scalar_is_the_fixed_order_sum(gpu, K):
    torch = gpu
    from rtx_nerf_amd import api
    api.set_deterministic(None, None)
    default = {case: _run(torch, api, K, case) for case in CASES}
    shadow = api.deterministic_shadow(64)
    api.set_deterministic(shadow, None)
    try:
        det = {case: _run(torch, api, K, case) for case in CASES}
        det2 = {case: _run(torch, api, K, case) for case in CASES}
        with pytest.raises(api._lib.RtxnError, match="reg->distortion"):      # the term is summed from the L_r stored there
            _run(torch, api, K, "l2_none3", outputs=False)
    finally:
        api.set_deterministic(None, None)
    for case in CASES:
        for k in default[case]:
            if k != "loss":                              # everything but the scalar is the default mode's, bit for bit
                assert np.array_equal(default[case][k].view(np.uint8), det[case][k].view(np.uint8)), (case, k)
            assert np.array_equal(det[case][k].view(np.uint8), det2[case][k].view(np.uint8)), (case, k)      # a second run: identical
    nh, idx, P, rad, step, ts, te, tgt, bg_np = case_inputs(K, "l2_none3")
    d = det["l2_none3"]
    want = _fixed_order_l2(d["pix"], tgt, d["dist"], LAMBDA_D)
    print(f"\n[K={K}] l2: deterministic {d['loss'][0]:.9e}, fp32 restatement {want:.9e}, default mode {default['l2_none3']['loss'][0]:.9e}")
    assert d["loss"][0] == want and want > 1e-3
    nh, idx, P, rad, step, ts, te, tgt, bg_np = case_inputs(K, "huber_constant4")
    d = det["huber_constant4"]
    p = d["pix"].astype(np.float64)
    l, _ = loss_terms("huber", p - _composited(bg_np, tgt))
    parts = (float(l.sum() / (3 * B_RAYS)),
             float(np.float32(LAMBDA_A)) / B_RAYS * float(((d["opa"].astype(np.float64) - tgt[:, 3].astype(np.float64)) ** 2).sum()),
             LAMBDA_D / B_RAYS * float(d["dist"].astype(np.float64).sum()))
    err = abs(float(d["loss"][0]) - sum(parts)) / sum(parts)
    print(f"[K={K}] huber + alpha + distortion {parts[0]:.6e} + {parts[1]:.6e} + {parts[2]:.6e}: deterministic {d['loss'][0]:.9e} "
          f"(rel {err:.2e}, bar {DET_BAR:.2e})")
    assert min(parts) > 1e-3 and err <= DET_BAR


# ---- 3. t plumbing -------------------------------------------------------------------------------------------------------------
def _sphere_occ(torch, R):
    from rtx_nerf_amd import scenes
    return torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()


def test_trainer_plumbs_the_traversals_distances(gpu):
    """A Trainer on a 32^3 grid, 512 rays.  The write pass's t_start / t_end for the lanes-per-ray the trainer chooses (for this
    launch and for a full batch) and for one lane per ray: identical bits; ascending and disjoint per ray; |start - o| and
    |end - o| within 1e-5; what Trainer._segments leaves in Trainer.t_start / t_end is the same; and the training compositor's
    depth on those buffers is rtxn_volrender_fwd_aux's within 1e-6 relative."""
    torch = gpu
    from rtx_nerf_amd import api, scenes
    from rtx_nerf_amd.train import Trainer, camera_rays
    R, n = 32, 512
    tr = Trainer(R, _sphere_occ(torch, R), encoding="freq", n_neurons=64, n_hidden_layers=2, batch_rays=n, max_segments=n * 48, lr=1e-2,
                 density_scale=120.0, mode="nerf", seed=3, distortion_weight=0.01)
    assert tr.t_start.shape == tr.t_end.shape == (n * 48,) and tr.distortion.shape == (n,)
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 32, 16)
    assert o.shape[0] == n
    tgt = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (n, 3)).astype(np.float32)).cuda()
    res = {}
    for sub in sorted({1, api.auto_sub_rays(n), tr.sub_rays}):
        kw = dict(grid_res=R, rays_o=o, rays_d=d, width=n, height=1, ray_begin=0, ray_count=n, occupancy=tr.occ, occupancy_coarse=tr.coarse,
                  occupancy_bricks=tr.bricks, occupancy_super=tr.super_mip, mode=api.TRACE_DDA, viewing_direction=tr.view_dirs,
                  num_hits=tr.num_hits, sub_rays=sub, sub_hits=tr.sub_hits)
        api.trace_grid(None, **kw)
        api.scan_hits(tr.num_hits[:n], tr.indices[:n], tr.total, tr.scan_ws)
        t0, t1 = torch.full((tr.max_segments,), -2.0, device="cuda"), torch.full((tr.max_segments,), -2.0, device="cuda")
        api.trace_grid(None, indices=tr.indices, start_points=tr.start, end_points=tr.end, seg_view=tr.seg_view, num_stored=tr.num_stored,
                       segment_capacity=tr.max_segments, t_start=t0, t_end=t1, **kw)
        torch.cuda.synchronize()
        P = int(tr.total.item())
        res[sub] = (P, t0[:P].cpu().numpy(), t1[:P].cpu().numpy(), tr.start[:P].cpu().numpy(), tr.end[:P].cpu().numpy(),
                    tr.num_stored[:n].cpu().numpy(), tr.indices[:n].cpu().numpy())
    P, t0, t1, sp, ep, ns, ix = res[1]
    assert P > n and P <= tr.max_segments and len(res) >= 2
    for sub, r in res.items():
        assert r[0] == P and np.array_equal(r[1].view(np.uint32), t0.view(np.uint32)) and np.array_equal(r[2].view(np.uint32), t1.view(np.uint32)), sub
    seg_ray = np.repeat(np.arange(n), ns)
    assert np.array_equal(ix, np.concatenate([[0], np.cumsum(ns)[:-1]]))
    assert np.all(t1 > t0) and np.all(t0 >= 0.0)
    same = seg_ray[1:] == seg_ray[:-1]
    assert same.sum() > n and np.all(t0[1:][same] >= t1[:-1][same])               # ascending, disjoint
    o_np = o.cpu().numpy().astype(np.float64)[seg_ray]
    e0 = np.abs(np.linalg.norm(sp - o_np, axis=1) - t0).max()
    e1 = np.abs(np.linalg.norm(ep - o_np, axis=1) - t1).max()
    # the trainer's own traversal, then its compositor: depth against the render path's
    tr.gradients(o, d, tgt)
    torch.cuda.synchronize()
    assert np.array_equal(tr.t_start[:P].cpu().numpy().view(np.uint32), t0.view(np.uint32))
    assert np.array_equal(tr.t_end[:P].cpu().numpy().view(np.uint32), t1.view(np.uint32))
    depth, depth_aux = torch.full((n,), -1.0, device="cuda"), torch.full((n,), -1.0, device="cuda")
    pix, lg, loss = torch.zeros((n, 3), device="cuda"), torch.zeros((n, 3), dtype=torch.float16, device="cuda"), torch.zeros(1, device="cuda")
    api.volrender_reg_train(tr.radiance, tr.t_vals, tr.num_stored, tr.indices, n, 32, tgt, tr.loss_scale, pix, lg, loss, torch.empty_like(tr.dout),
                            None, None, api.train_regularizer(0.0, tr.t_start, tr.t_end, depth=depth))
    api.volrender_fwd_aux(tr.radiance, tr.t_vals, tr.num_stored, tr.indices, n, 32, torch.zeros((n, 3), device="cuda"), mode=api.VR_NERF,
                          sample_type=api.SAMPLING_MIDPOINT_WORLD, t_start=tr.t_start, t_end=tr.t_end, depth=depth_aux)
    torch.cuda.synchronize()
    a, b = depth.cpu().numpy().astype(np.float64), depth_aux.cpu().numpy().astype(np.float64)
    hit = ns > 0
    rel = (np.abs(a - b)[hit] / np.abs(b[hit])).max()
    print(f"\nsub_rays {sorted(res)}: {P} segments; | |start - o| - t_start | max {e0:.2e}, | |end - o| - t_end | max {e1:.2e}; "
          f"training depth vs rtxn_volrender_fwd_aux: max rel {rel:.2e} (depth up to {b.max():.3f})")
    assert e0 <= 1e-5 and e1 <= 1e-5
    assert np.all(a[~hit] == 0.0) and np.all(b[hit] > 0.0)
    assert rel <= 1e-6
    assert float(tr.distortion[:n].max()) > 0.0


# ---- 4. the three stepping paths ------------------------------------------------------------------------------------------------
STEP_LAMBDA, STEP_LS = 0.5, 4096.0            # three steps on random targets: a weight that moves the parameters at once


def _small_trainer(torch, encoding, seed=3, **kw):
    """tests/test_gpu_train_loss.py's _small_trainer, with the loss scale free"""
    from rtx_nerf_amd.train import Trainer
    R, B = 16, 900
    hgd = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
    kw.setdefault("loss_scale", STEP_LS)
    return Trainer(R, _sphere_occ(torch, R), encoding=encoding, n_neurons=64, n_hidden_layers=4 if encoding == "hash" else 2,
                   hashgrid=hgd if encoding == "hash" else None, n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2,
                   density_scale=120.0, mode="nerf", seed=seed, **kw)


_BATCHES = {}


def _batches(torch, n):
    if n not in _BATCHES:
        from rtx_nerf_amd import scenes
        from rtx_nerf_amd.train import camera_rays
        focal = scenes.lego_focal_length(True)
        rng = np.random.default_rng(8)
        out = []
        for i in range(n):
            o, d = camera_rays(scenes.pose_spherical(25.0 + 55.0 * i, -28.0 + 4.0 * i, origin_scale=10.0), focal, 30, 30)
            out.append((o, d, torch.from_numpy(rng.uniform(0, 1, (900, 3)).astype(np.float32)).cuda()))
        _BATCHES[n] = out
    return _BATCHES[n]


@pytest.mark.parametrize("encoding,jitter", [("hash", False), ("hash", True), ("freq", True)])
def test_eager_captured_and_one_call_steps_agree(gpu, encoding, jitter):
    """step(), step_captured() and step_entry() with distortion_weight > 0, deterministic mode: the same loss scalar, L_r and
    parameters after each of three steps, bit for bit -- with the samples at their midpoints and jittered.  A trainer without
    the regulariser ends elsewhere."""
    torch = gpu
    kw = dict(deterministic=True, sample_jitter=jitter, jitter_seed=11, distortion_weight=STEP_LAMBDA)
    a, b, c = (_small_trainer(torch, encoding, **kw) for _ in range(3))
    b.capture_step(900, launch_segments=900 * 30)
    c.entry_args(900, launch_segments=900 * 30)
    for i, (o, d, t) in enumerate(_batches(torch, 3)):
        la = a.step(o, d, t).clone()
        da = a.distortion.clone()
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        lb = b.step_captured().clone()
        db = b.distortion.clone()
        c.graph_rays_o.copy_(o); c.graph_rays_d.copy_(d); c.graph_targets.copy_(t)
        lc = c.step_entry().clone()
        torch.cuda.synchronize()
        P = int(a.total.item())
        assert float(da.max()) > 0.0 and float(la) > 0.0
        for name, x, lx, dx in (("captured", b, lb, db), ("one-call", c, lc, c.distortion)):
            assert torch.equal(a.t_start[:P], x.t_start[:P]) and torch.equal(a.t_end[:P], x.t_end[:P]), (name, i)
            assert torch.equal(da, dx), (name, i)
            assert torch.equal(la, lx), (name, i, float(la), float(lx))
            assert torch.equal(a.params, x.params) and torch.equal(a.master, x.master), (name, i)
    assert a.step_count == b.step_count == c.step_count == 3
    plain = _small_trainer(torch, encoding, deterministic=True, sample_jitter=jitter, jitter_seed=11)
    assert plain.distortion is None and plain.t_start is None and plain._reg is None
    for o, d, t in _batches(torch, 3):
        plain.step(o, d, t)
    assert not torch.equal(plain.master, a.master)


@pytest.mark.parametrize("encoding", ["hash", "freq"])
def test_eager_captured_and_one_call_steps_agree_in_default_mode(gpu, encoding):
    """The same three paths with the float atomics of default mode (the loss scalar included), at the bars
    tests/test_gpu_train_loss.py holds its losses to: 5e-4 on the loss of every step, 3e-2 on the parameters' norm at the end."""
    torch = gpu
    a, b, c = (_small_trainer(torch, encoding, distortion_weight=STEP_LAMBDA) for _ in range(3))
    b.capture_step(900, launch_segments=900 * 30)
    c.entry_args(900, launch_segments=900 * 30)
    for i, (o, d, t) in enumerate(_batches(torch, 4)):
        la = float(a.step(o, d, t).item())
        da = a.distortion.clone()
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        lb = float(b.step_captured().item())
        db = b.distortion.clone()
        c.graph_rays_o.copy_(o); c.graph_rays_d.copy_(d); c.graph_targets.copy_(t)
        lc = float(c.step_entry().item())
        assert abs(la - lb) <= 5e-4 * abs(la) and abs(la - lc) <= 5e-4 * abs(la), (i, la, lb, lc)
        assert float(da.max()) > 0.0
        for dx in (db, c.distortion):
            assert float((da - dx).abs().max()) <= 5e-4 * float(da.max()), i
    assert a.step_count == b.step_count == c.step_count == 4
    pa = a.master.cpu().numpy()
    for x in (b, c):
        assert np.linalg.norm(pa - x.master.cpu().numpy()) <= 3e-2 * np.linalg.norm(pa)


def test_prefetched_captured_steps_agree_with_eager(gpu):
    """capture_step(prefetch=True): batch k + 1 is traversed into the second buffer set -- with t_start / t_end and a regulariser
    struct of its own -- beside the gradient kernels of batch k.  Deterministic mode: the losses, one call later, and the
    parameters after flush_captured() are the eager trainer's bit for bit; five batches, so both sets train."""
    torch = gpu
    kw = dict(deterministic=True, distortion_weight=STEP_LAMBDA)
    a, b = _small_trainer(torch, "hash", **kw), _small_trainer(torch, "hash", **kw)
    b.capture_step(900, launch_segments=900 * 30, prefetch=True)
    assert len(b._g_sets) == 2 and b._g_sets[1]["reg"] is not b._g_sets[0]["reg"]
    assert b._g_sets[1]["t_start"].data_ptr() != b.t_start.data_ptr()
    eager = [a.step(o, d, t).clone() for o, d, t in _batches(torch, 5)]
    got = []
    for o, d, t in _batches(torch, 5):
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        r = b.step_captured()
        got.append(None if r is None else r.clone())
    assert got[0] is None and b.step_count == 4
    got = got[1:] + [b.flush_captured().clone()]
    torch.cuda.synchronize()
    assert b.step_count == 5 and b.flush_captured() is None and b.truncated_steps == 0
    for i, (x, y) in enumerate(zip(eager, got)):
        assert float(x) > 0.0 and torch.equal(x, y), (i, float(x), float(y))
    assert torch.equal(a.master, b.master) and torch.equal(a.distortion, b.distortion)
    assert float(b._g_sets[1]["t_end"].max()) > 0.0


def test_drawn_batches_eager_and_captured_agree(gpu):
    """attach_images(): step_images() and capture_step(draw=True) with the regulariser, deterministic mode, bit for bit"""
    torch = gpu
    from rtx_nerf_amd import api, scenes
    rng = np.random.default_rng(5)
    frames = rng.uniform(0, 1, (3, 24, 24, 3)).astype(np.float32)
    poses = np.stack([np.asarray(scenes.pose_spherical(35.0 + 110.0 * i, -25.0 - 10.0 * i, origin_scale=10.0), np.float32).reshape(16)
                      for i in range(3)])
    iset = api.ImageSet(torch.from_numpy(frames).cuda(), torch.from_numpy(poses).cuda(), scenes.lego_focal_length(True))
    a = _small_trainer(torch, "hash", deterministic=True, distortion_weight=STEP_LAMBDA).attach_images(iset)
    b = _small_trainer(torch, "hash", deterministic=True, distortion_weight=STEP_LAMBDA).attach_images(iset)
    b.capture_step(900, launch_segments=900 * 30, draw=True)
    for i in range(3):
        la = a.step_images().clone()
        lb = b.step_captured().clone()
        torch.cuda.synchronize()
        assert torch.equal(a.drawn[:900], b.drawn[:900])
        assert float(la) > 0 and torch.equal(la, lb), (i, float(la), float(lb))
        assert torch.equal(a.distortion, b.distortion) and float(a.distortion.max()) > 0.0
        assert torch.equal(a.master, b.master), i
    assert a.draw_count == b.draw_count == 3


# ---- 6. it regularises -----------------------------------------------------------------------------------------------------------
# Measured on an MI355X (tools/distortion_sweep.py; profiles/r10/distortion_sweep.txt), 300 steps at loss_scale 4096.  Without the regulariser: mean L_r over
# the held-out pose 2.35e-2, held-out PSNR 25.33 dB.  With distortion_weight 0.01: 9.5e-3 (0.40 of it) and 26.53 dB; 0.003 gives
# 0.63 of it, 0.03 gives 0.24 at 24.61 dB, and from 0.1 on the term outweighs the colour loss (2e-5 at the end) and the model goes
# transparent (13.7 dB).  The bars: L_r below 0.7 of the unregularised run's, between what 0.003 and 0.01 reach, and a PSNR no more
# than 1 dB below the unregularised run's, which 0.03 already misses on the other side.
TRAIN_LAMBDA, TRAIN_LS = 0.01, 4096.0
E2E_L_RATIO = 0.7
E2E_PSNR_MARGIN = 1.0


def test_training_with_the_regulariser(gpu):
    """The sphere teacher of the loss tests (tools/train_demo.py: 300 steps, hash model, seed 0), without the regulariser and with
    distortion_weight = 0.01 at loss_scale = 4096, both runs at that loss scale.  The mean L_r over the held-out pose's 4096 rays
    ends lower with the regulariser on, and the held-out PSNR stays within a margin of the unregularised run: see E2E_L_RATIO and
    E2E_PSNR_MARGIN above."""
    torch = gpu
    import distortion_sweep
    import train_demo
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    o, d = camera_rays(scenes.pose_spherical(77.0, -33.0, origin_scale=10.0), scenes.lego_focal_length(True), 64, 64)
    res = {}
    for name, lam in (("off", 0.0), ("on", TRAIN_LAMBDA)):
        L = {}

        def probe(tr, rays_o, rays_d, targets, when):
            L[when] = distortion_sweep.mean_distortion(tr, o, d)

        p0, p1, losses = train_demo.run(steps=300, encoding="hash", verbose=False, probe=probe, distortion_weight=lam, loss_scale=TRAIN_LS)
        res[name] = (p1, L["before"], L["after"], losses[-1])
        print(f"\ndistortion_weight {lam}, loss_scale {TRAIN_LS}: held-out PSNR {p0:.2f} -> {p1:.2f} dB, mean L_r {L['before']:.4e} -> "
              f"{L['after']:.4e}, last loss {losses[-1]:.4e}")
    assert res["on"][2] < E2E_L_RATIO * res["off"][2], res
    assert res["on"][0] > res["off"][0] - E2E_PSNR_MARGIN and res["off"][0] > 20.0, res

