"""The backward and fused training compositors on the GPU against float64, element by element, over the ray ladder of
tests/_compositor_float64.py: every length either side of a lane, sub-block (128) and step (512) boundary up to the documented
longest ray of 4096 samples, in six density regimes, all in one batch per K; batches of 1 and 5 rays; tails and sentinels.

One test per (entry point, K).  Which kernel form a call takes cannot be observed from outside, so every test restates the
launcher's condition (even K, step lengths 8-byte aligned, gradients 16-byte aligned: the pair schedule) on the very pointers it
hands over and asserts the form it was written for:
    launch_volrender_backward_cuda NERF   volrender_l2_fused_multi_kernel<4> (target == NULL) | volrender_bwd_nerf_kernel
    launch_volrender_backward_cuda COMPAT volrender_bwd_compat_kernel
    volrender_l2_train                    volrender_l2_fused_multi_kernel<4> | volrender_l2_fused_kernel
    volrender_l2_train_ex                 volrender_l2_bg_multi_kernel<4> | volrender_l2_bg_kernel
    volrender_loss_train                  composite_train_multi_kernel<false, 4> | composite_train_kernel<false>
    volrender_reg_train                   composite_train_multi_kernel<true, 4> | composite_train_kernel<true>

The bars: radiance gradients within the derived per-element bound of _compositor_float64 (no element left out); COMPAT within one
fp16 ulp of the float64 formula; pixels and opacities within 3e-6; the loss within 2e-6 relative (1e-5 with the regulariser, the
existing bars); fp16 loss gradients within one ulp of half(LS dl / (3 B)), and different from it only where the float64 value
lies within the pixels' bar (through dl/dp) of the rounding boundary.

Measured on an MI355X (profiles/r23/compositor_float64.txt): every case inside the bound, no defect found.  The largest err / bound
reaches 0.99-1.00 in every ladder case and it is the fp16 rounding term: a stored value is the fp32 value rounded to nearest, half an ulp by
construction.  The fp32 part of the bound, the one the counts k stand behind, is used to at most 0.19 (the third figure of every
printed line: the largest fp32 error the stored values prove, over the fp32 part; benign rays, where 1 - expf(-x) loses expf's
ulp absolutely); pixels and opacities within 1.6e-7, the loss within 1.9e-7 relative, at most one fp16 loss gradient per case
different from half(float64) and that one at a rounding boundary; COMPAT never more than one ulp, 99.98 % equal."""
import faulthandler
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _compositor_float64 as cf                                   # noqa: E402

LS = 128.0
COLOR = (0.9, 0.25, 1.0)
LAMBDA_A, LAMBDA_D = 0.5, 1.0
DELTA = np.float32(0.1)                                 # api.train_loss("huber")'s default
PAD = 64                                                # elements allocated past the pixels and the loss gradients
_DETERMINISTIC = []                                     # a test that registered a deterministic workspace says so here


@pytest.fixture(autouse=True)
def _own_timeout_and_default_mode():
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    if _DETERMINISTIC:
        from rtx_nerf_amd import api
        api.set_deterministic(None, None)
        _DETERMINISTIC.clear()


def _dev(torch, b, misaligned=False):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d = dict(rad=t(b.rad), step=t(b.step), nh=t(b.nh), idx=t(b.idx), ts=t(b.ts), te=t(b.te))
    if misaligned:                                         # a view that starts 4 bytes into its allocation
        d["step"] = torch.cat([torch.zeros(1, device="cuda"), d["step"]])[1:]
        assert d["step"].data_ptr() % 8 == 4 and d["step"].is_contiguous()
    return d


def _half_buffer(torch, n):
    """n fp16 elements, every one the sentinel pattern"""
    return torch.full((n,), cf.SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16)


def _form(K, step, out):
    """the launchers' condition (volrender.hip, composite_train.hip), on the pointers of this call"""
    return "pair" if K % 2 == 0 and step.data_ptr() % 8 == 0 and out.data_ptr() % 16 == 0 else "one"


def _report(title, table):
    print()
    for line in cf.table_lines(title, table):
        print(line)


CASES_BWD = [(32, False), (2, False), (6, False), (130, False), (1, False), (7, False), (32, True)]


# ---- 1. the backward with the pixel gradients given ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,misaligned", CASES_BWD)
def test_backward_nerf_with_given_gradients(gpu, K, misaligned):
    """fp16 N(0, 1) pixel gradients.  Even K: volrender_l2_fused_multi_kernel<4> in its target == NULL branch; odd K, and K = 32
    with the step lengths 4 bytes off an 8-byte boundary: volrender_bwd_nerf_kernel (S summed per sample: below the same k_S)."""
    torch = gpu
    from rtx_nerf_amd import api
    b = cf.ladder(K)
    g16 = np.random.default_rng(100 + K).standard_normal((b.B, 3)).astype(np.float16)
    dev = _dev(torch, b, misaligned)
    lg = torch.from_numpy(g16).cuda()
    out = _half_buffer(torch, (b.N + cf.TAIL) * 4).view(b.N + cf.TAIL, 4)
    form = _form(K, dev["step"], out)
    assert form == ("pair" if K % 2 == 0 and not misaligned else "one")
    api.launch_volrender_backward_cuda(None, lg, dev["rad"], dev["step"], dev["nh"], dev["idx"], b.B, K, out, mode=api.VR_NERF)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(lg.cpu().numpy().view(np.uint16), g16.view(np.uint16))          # the given gradients are read only
    cf.check_written(got, b.N)
    ref = cf.gradients(b, g16.astype(np.float64), form)
    table = cf.check_elements(f"bwd NERF K={K} {form}", got[:b.N], ref.ref, ref.bound, b)
    _report(f"bwd NERF K={K}{' misaligned' if misaligned else ''} ({form})", table)
    assert np.abs(ref.ref[:, 3]).max() > 1e-2 and np.abs(ref.ref[:, :3]).max() > 1e-2


@pytest.mark.parametrize("K", [32, 1, 7])
def test_backward_compat_within_one_ulp(gpu, K):
    """volrender_bwd_compat_kernel with the sampler's REGULAR t_vals and with jittered ones: the reference project's per-sample
    formula, t carried over steps and segment boundaries, never reset inside a ray"""
    torch = gpu
    from rtx_nerf_amd import api
    b = cf.ladder(K)
    g16 = np.random.default_rng(200 + K).standard_normal((b.B, 3)).astype(np.float16)
    dev = _dev(torch, b)
    lg = torch.from_numpy(g16).cuda()
    for name in ("t_regular", "t_jitter"):
        t = getattr(b, name)
        out = _half_buffer(torch, (b.N + cf.TAIL) * 4).view(b.N + cf.TAIL, 4)
        api.launch_volrender_backward_cuda(None, lg, dev["rad"], torch.from_numpy(t).cuda(), dev["nh"], dev["idx"], b.B, K, out,
                                           mode=api.VR_COMPAT)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        cf.check_written(got, b.N)
        ref = cf.compat_backward(b, g16.astype(np.float64), t)
        ulps = cf.compat_ulps(got[:b.N], ref)
        print(f"\nmeasured bwd COMPAT K={K} {name}: max {int(ulps.max())} ulp, equal to half(float64) {(ulps == 0).mean():.5f}")
        assert np.isfinite(got[:b.N].astype(np.float32)).all() and ulps.max() <= 1
        assert np.abs(ref).max() > 1e-2


# ---- 2. the fused training entries ---------------------------------------------------------------------------------------------------
def _train(torch, entry, b, misaligned=False, deterministic=False, title=""):
    """entry: "l2" (RGB targets, no background), "l2_ex" (constant background, RGBA targets), "loss" (Huber + the alpha term, an
    opacity buffer), "reg" (the same with the distortion regulariser).  Every output buffer is pre-filled and has a tail."""
    from rtx_nerf_amd import api
    K, B, N = b.K, b.B, b.N
    kind = "l2" if entry in ("l2", "l2_ex") else "huber"
    lam_a = LAMBDA_A if entry in ("loss", "reg") else 0.0
    lam_d = LAMBDA_D if entry == "reg" else 0.0
    tgt = np.ascontiguousarray(b.tgt[:, :3]) if entry == "l2" else b.tgt
    bg_np = np.zeros((B, 3), np.float32) if entry == "l2" else np.tile(np.array(COLOR, np.float32), (B, 1))
    dev = _dev(torch, b, misaligned)
    tgt_d = torch.from_numpy(tgt).cuda()
    pix = torch.full((3 * B + PAD,), float(cf.F32_SENTINEL), device="cuda")
    lg = _half_buffer(torch, 3 * B + PAD)
    loss = torch.full((1,), 9.0, device="cuda")           # a stale value: the call must replace it
    out = _half_buffer(torch, (N + cf.TAIL) * 4).view(N + cf.TAIL, 4)
    opa, dist, dep = (torch.full((B + PAD,), float(cf.F32_SENTINEL), device="cuda") for _ in range(3))
    form = _form(K, dev["step"], out)
    assert form == ("pair" if K % 2 == 0 and not misaligned else "one")
    if deterministic:
        _DETERMINISTIC.append(True)
        api.set_deterministic(api.deterministic_shadow(64), None)
    args = (dev["rad"], dev["step"], dev["nh"], dev["idx"], B, K, tgt_d, LS, pix, lg, loss, out)
    bg = None if entry == "l2" else api.train_background(COLOR, target_channels=4)
    spec = api.train_loss(kind, opacity_weight=lam_a, opacity=opa) if entry in ("loss", "reg") else None
    if entry == "l2":
        api.volrender_l2_train(*args)
    elif entry == "l2_ex":
        api.volrender_l2_train_ex(*args, bg)
    elif entry == "loss":
        api.volrender_loss_train(*args, bg, spec)
    else:
        api.volrender_reg_train(*args, bg, spec, api.train_regularizer(lam_d, dev["ts"], dev["te"], dist, dep))
    torch.cuda.synchronize()
    pix_np, lg_np, got = pix.cpu().numpy(), lg.cpu().numpy(), out.cpu().numpy()
    opa_np, dist_np, dep_np = opa.cpu().numpy(), dist.cpu().numpy(), dep.cpu().numpy()

    # tails untouched, everything in range written
    assert np.all(pix_np[3 * B:] == cf.F32_SENTINEL) and np.all(pix_np[:3 * B] != cf.F32_SENTINEL)
    assert cf.is_sentinel(lg_np[3 * B:]).all() and not cf.is_sentinel(lg_np[:3 * B]).any()
    cf.check_written(got, N)
    for buf, used in ((opa_np, entry in ("loss", "reg")), (dist_np, entry == "reg"), (dep_np, entry == "reg")):
        assert np.all(buf[B:] == cf.F32_SENTINEL) and np.all((buf[:B] != cf.F32_SENTINEL) == used)
    pix_np, lg_np = pix_np[:3 * B].reshape(B, 3), lg_np[:3 * B].reshape(B, 3)

    # forward: pixels, opacities, the loss scalar, the fp16 loss gradients
    fwd = cf.gradients(b, np.zeros((B, 3)), form, bg=bg_np, reg_k=0.0)
    empty = b.nh == 0
    assert np.array_equal(pix_np[empty], bg_np[empty])                                   # pixel = background exactly
    pix_err = np.abs(pix_np - fwd.pix).max()
    assert pix_err <= 3e-6, pix_err
    alpha = tgt[:, 3].astype(np.float64) if tgt.shape[1] == 4 else np.zeros(B)
    A_err = 0.0
    if entry in ("loss", "reg"):
        assert np.all(opa_np[:B][empty] == 0.0)
        A_err = np.abs(opa_np[:B] - fwd.A).max()
        assert A_err <= 3e-6, A_err
    e = fwd.pix - cf.composited_target(bg_np, tgt)
    l, dl = cf.loss_terms(kind, e, fwd.pix, float(DELTA))
    want_lg = LS * dl / (3 * B)
    slack = LS * cf.LIPSCHITZ[kind] * 3e-6 / (3 * B) + 5 * cf.U * np.abs(want_lg)
    differ, _ = cf.check_loss_gradients(lg_np, want_lg, slack)

    # radiance gradients: the kernel's own fp16 g, and g_A recomputed from the kernel's own A by the kernel's operations
    gA = None
    if lam_a > 0.0:
        inv_rays = np.float32(1.0) / np.float32(B)
        gA = (np.float32(LS) * (np.float32(lam_a) * (np.float32(2.0) * (opa_np[:B] - alpha.astype(np.float32)))) * inv_rays).astype(np.float16)
        assert gA.dtype == np.float16
        gA = gA.astype(np.float64)
    k = float(np.float32(LS) * np.float32(lam_d) / np.float32(B)) if lam_d else 0.0
    ref = cf.gradients(b, lg_np.astype(np.float64), form, bg=None if entry == "l2" else bg_np, gA=gA, reg_k=k)
    ref_loss = float(l.sum() / (3 * B) + float(np.float32(lam_a)) / B * ((fwd.A - alpha) ** 2).sum() * (lam_a > 0) + lam_d / B * ref.L.sum())
    loss_err = abs(float(loss.item()) - ref_loss) / ref_loss
    table = cf.check_elements(f"{entry} K={K} B={B} {form}", got[:N], ref.ref, ref.bound, b)
    _report(f"{title or entry} K={K} B={B}{' misaligned' if misaligned else ''}{' deterministic' if deterministic else ''} ({form})", table)
    print(f"measured {title or entry} K={K} B={B}: pixels max|err| {pix_err:.2e}  opacity max|err| {A_err:.2e}  loss rel {loss_err:.2e}  "
          f"fp16 loss gradients differing from half(float64) {differ} of {3 * B}")
    assert ref_loss > 1e-3 and loss_err < (1e-5 if entry == "reg" else 2e-6), (ref_loss, loss_err)
    assert np.abs(ref.ref[:, 3]).max() > 1e-3 and np.abs(ref.ref[:, :3]).max() > 1e-3
    if entry == "reg":
        assert np.all(dist_np[:B][empty] == 0.0) and np.all(dep_np[:B][empty] == 0.0)
        m, _ = cf.midpoints(b)
        m_max = np.array([m[s].max() if s.stop > s.start else 1.0 for s in cf.ray_slices(b)])
        depth_ratio = (np.abs(dep_np[:B] - ref.depth) / (3e-6 * m_max)).max()
        L_err = np.abs(dist_np[:B] - ref.L).max() / ref.L.max()
        plain = cf.gradients(b, lg_np.astype(np.float64), form, bg=bg_np, gA=gA)
        moved = (np.abs(ref.ref[:, 3] - plain.ref[:, 3]) > ref.bound[:, 3])[ref.ref[:, 3] != 0].mean()
        print(f"measured {entry} K={K}: depth max err / (3e-6 max m) {depth_ratio:.3f}  L_r max|err| / max L_r {L_err:.2e}  the term moves "
              f"{moved:.3f} of the non-zero sigma-gradients by more than their bound")
        assert depth_ratio <= 1.0 and L_err <= 2e-5
        assert moved >= 0.25                                  # without the term the test cannot pass


@pytest.mark.parametrize("K", [32, 2, 6, 1, 7])
def test_l2_train(gpu, K):
    """volrender_l2_fused_multi_kernel<4> (even K), the default training kernel, and volrender_l2_fused_kernel (odd K)"""
    _train(gpu, "l2", cf.ladder(K))


@pytest.mark.parametrize("K", [32, 2, 7])
def test_l2_train_over_a_background(gpu, K):
    """volrender_l2_bg_multi_kernel<4> and volrender_l2_bg_kernel: constant background, RGBA targets"""
    _train(gpu, "l2_ex", cf.ladder(K))


@pytest.mark.parametrize("K", [32, 2, 7])
def test_loss_train_huber_and_alpha(gpu, K):
    """composite_train_multi_kernel<false, 4> and composite_train_kernel<false>: Huber, lambda = 0.5, an opacity buffer"""
    _train(gpu, "loss", cf.ladder(K))


@pytest.mark.parametrize("K", [32, 7])
def test_reg_train(gpu, K):
    """composite_train_*<true>: the row above with the distortion regulariser, lambda_d = 1, ascending disjoint segments"""
    _train(gpu, "reg", cf.ladder(K))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("entry", ["l2", "l2_ex", "loss"])
def test_batches_that_end_inside_a_block(gpu, entry, B):
    """1 and 5 rays at K = 32: the last block has idle waves while the per-block loss reduction runs"""
    _train(gpu, entry, cf.small(B))


def test_l2_train_in_deterministic_mode(gpu):
    """the default kernel without a loss pointer and the fixed-order sum behind it: every bar of test_l2_train"""
    _train(gpu, "l2", cf.ladder(32), deterministic=True)


def test_l2_train_misaligned_step_lengths(gpu):
    """K = 32 with the step lengths 4 bytes off an 8-byte boundary: volrender_l2_fused_kernel over rays of up to 64 steps"""
    _train(gpu, "l2", cf.ladder(32), misaligned=True)
