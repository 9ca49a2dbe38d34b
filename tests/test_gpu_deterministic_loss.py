"""The loss scalar of rtxn_volrender_l2_train[_ex] in deterministic mode (loss.hip): with a deterministic workspace registered
the compositor is launched without a loss pointer and a one-block kernel sums the per-ray terms in a fixed order.  Checked
here against a float64 restatement from the call's own `pixels` and `targets` -- 3-channel targets, straight RGBA over a
constant and over a random background -- against the default-mode scalar of the same call, and for identical bits on a second run.

Shapes: 777 rays (not a multiple of 4: the last group holds one ray) with K = 32 (four rays per block) and K = 7 (the
one-ray-per-wave compositor), and 5001 rays (more than 4096: the 1251 groups exceed the block's 1024 threads, so threads 0..226
add two groups each; again a last group of one ray).

The bound.  The restatement forms each ray's target in float32 with the kernel's own operations (a * c + (1 - a) * bg, no
contraction), so d = pixel - target carries one rounding; d*d three times, two additions and the product with 1 / (3 n) make six
more at the most, and 1 / (3 n) is itself rounded: at most 8 roundings per term.  All terms are >= 0, so every addition of
the sum costs at most one further relative rounding on the path of any term: 2 inside a group of four, ceil(groups / 1024) <= 2
in a thread, 10 in the tree over 1024 threads = 14.  (1 + 2^-24)^22 - 1 < 24 * 2^-24 = 1.43e-6 relative, at any of these sizes.
The default-mode scalar sums the same terms with float atomics in whatever order the blocks retire: m atomics (one per block of
four rays, or one per ray for odd K) cost any term at most m roundings, with the 8 of the term and 2 inside a block
(m + 10) * 2^-24 (with the slack of the first bound), and the two modes differ by at most the sum of the two bars.  That bar
is the worst case of an unordered sum, hence loose (5e-5 at 777 atomics); the figures are printed."""
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DET_BAR = 24 * 2.0 ** -24


def _fmix32(h):
    h = np.asarray(h, np.uint32)
    with np.errstate(over="ignore"):
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
        h = h ^ (h >> np.uint32(16))
    return h


def random_backgrounds(seed, step, n):
    """float32[n][3]: the RANDOM background of rays 0..n-1 (include/rtxn.h), restated in numpy"""
    with np.errstate(over="ignore"):
        h0 = _fmix32(np.uint32(seed) + np.uint32(0x9E3779B9) * np.uint32(step & 0xFFFFFFFF))
    r = np.arange(n, dtype=np.uint32)[:, None] * np.uint32(3) + np.arange(3, dtype=np.uint32)[None, :]
    return (_fmix32(h0 ^ r) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _batch(rng, B, K):
    nh = rng.integers(0, 8, B).astype(np.int32)
    nh[::7] = 0                                       # rays without segments
    nh[3::50] = rng.integers(17, 40, nh[3::50].size)  # rays longer than 512 samples
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
    P = int(nh.sum())
    rad = np.concatenate([rng.uniform(0, 1, (P * K, 3)), rng.uniform(0, 1.5, (P * K, 1))], 1).astype(np.float32)
    step = rng.uniform(0.0, 0.2, P * K).astype(np.float32)
    return nh, idx, P, rad, step


@pytest.fixture(autouse=True)
def _own_timeout():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _restated_loss(pix, tgt, bg_np):
    """float64 sum over rays and channels of (pixel - target)^2 / (3 n); RGBA targets composited in float32 as include/rtxn.h defines"""
    if tgt.shape[1] == 4:
        a = tgt[:, 3:4]
        t = a * tgt[:, :3] + (np.float32(1.0) - a) * bg_np
        assert t.dtype == np.float32
    else:
        t = tgt
    d = pix.astype(np.float64) - t.astype(np.float64)
    return float((d ** 2).sum() / (3 * pix.shape[0]))


def _run(torch, api, dev, B, K, P, ls, bg):
    pix = torch.zeros((B, 3), device="cuda")
    lg = torch.zeros((B, 3), dtype=torch.float16, device="cuda")
    loss = torch.full((1,), 9.0, device="cuda")           # a stale value: the call must replace it, not add to it
    out = torch.zeros((P * K, 4), dtype=torch.float16, device="cuda")
    if bg is None:
        api.volrender_l2_train(dev["rad"], dev["step"], dev["nh"], dev["idx"], B, K, dev["tgt"], ls, pix, lg, loss, out)
    else:
        api.volrender_l2_train_ex(dev["rad"], dev["step"], dev["nh"], dev["idx"], B, K, dev["tgt"], ls, pix, lg, loss, out, bg)
    torch.cuda.synchronize()
    return loss.cpu().numpy().copy(), pix.cpu().numpy(), lg.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("B,K", [(777, 32), (777, 7), (5001, 32)])
@pytest.mark.parametrize("case", ["plain3", "constant4", "random4"])
def test_deterministic_loss_against_restatement_and_default_mode(gpu, case, B, K):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(B * 31 + K * 7 + len(case))
    ls = 128.0
    nh, idx, P, rad, step = _batch(rng, B, K)
    tc = 3 if case == "plain3" else 4
    tgt = rng.uniform(0, 1, (B, tc)).astype(np.float32)
    if tc == 4:
        tgt[::5, 3] = 0.0
        tgt[1::5, 3] = 1.0
    step_d = None
    if case == "plain3":
        bg, bg_np = None, None
    elif case == "constant4":
        color = (0.9, 0.25, 1.0)
        bg_np = np.tile(np.array(color, np.float32), (B, 1))
        bg = api.train_background(color, target_channels=4)
    else:
        step_d = torch.full((1,), 41, dtype=torch.int32, device="cuda")
        bg_np = random_backgrounds(2024, 41, B)
        bg = api.train_background("random", seed=2024, step=step_d, target_channels=4)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(rad=rad, step=step, nh=nh, idx=idx, tgt=tgt).items()}

    api.set_deterministic(None, None)
    default = _run(torch, api, dev, B, K, P, ls, bg)
    shadow = api.deterministic_shadow(64)
    api.set_deterministic(shadow, None)
    try:
        det1 = _run(torch, api, dev, B, K, P, ls, bg)
        det2 = _run(torch, api, dev, B, K, P, ls, bg)
    finally:
        api.set_deterministic(None, None)

    ref = _restated_loss(det1[1], tgt, bg_np)
    DEFAULT_BAR = ((B + 3) // 4 if K % 2 == 0 else B) * 2.0 ** -24 + DET_BAR * 10 / 24
    det_err = abs(float(det1[0][0]) - ref) / ref
    default_err = abs(float(default[0][0]) - ref) / ref
    modes = abs(float(det1[0][0]) - float(default[0][0])) / ref
    print(f"\n[{case} B={B} K={K}] float64 restatement {ref:.9e}  deterministic {det1[0][0]:.9e} (rel {det_err:.2e}, bar {DET_BAR:.2e})  "
          f"default {default[0][0]:.9e} (rel {default_err:.2e}, bar {DEFAULT_BAR:.2e})  between the modes {modes:.2e}")
    assert ref > 1e-3                                           # a loss worth summing
    # everything but the scalar is the default mode's, bit for bit: the compositor only lost its loss pointer
    for a, b in zip(default[1:], det1[1:]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert det_err <= DET_BAR
    assert default_err <= DEFAULT_BAR
    assert modes <= DET_BAR + DEFAULT_BAR
    # a second run: identical bits, scalar included
    for a, b in zip(det1, det2):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
