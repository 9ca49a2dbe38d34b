"""The float64 restatement of rtxn_image_metrics (tests/_image_metrics_float64.py) against the definition and its closed forms,
on the CPU: what the GPU tests then hold the kernel to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_metrics_float64 as M  # noqa: E402


def _pair(h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((h, w, 3))
    return x, np.clip(x + 0.1 * rng.standard_normal((h, w, 3)), 0.0, 1.0)


@pytest.mark.parametrize("w,h", [(11, 11), (37, 29)])
def test_separable_form_equals_the_direct_window_loop(w, h):
    x, y = _pair(h, w, 1)
    assert abs(M.ssim(x, y) - M.ssim_direct(x, y)) <= 1e-12
    near_white = 1.0 - np.random.default_rng(2).integers(0, 3, (h, w, 3)) / 255.0
    other = 1.0 - np.random.default_rng(3).integers(0, 3, (h, w, 3)) / 255.0
    assert abs(M.ssim(near_white, other) - M.ssim_direct(near_white, other)) <= 1e-12


def test_window_is_normalised_and_symmetric():
    w = M.window()
    assert w.shape == (11,) and abs(w.sum() - 1.0) <= 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == 5
    assert abs(w[4] / w[5] - np.exp(-1.0 / 4.5)) <= 1e-15


@pytest.mark.parametrize("a,b", [(0.3, 0.7), (1.0, 0.0), (0.5, 0.5), (0.0, 0.0)])
def test_constant_pair_closed_form(a, b):
    x, y = np.full((13, 17, 3), a), np.full((13, 17, 3), b)
    assert abs(M.ssim(x, y) - (2 * a * b + M.C1) / (a * a + b * b + M.C1)) <= 1e-12


def test_identity_bound_and_symmetry():
    x, y = _pair(29, 37, 4)
    assert abs(M.ssim(x, x) - 1.0) <= 1e-12
    assert M.ssim_map(x, y).max() <= 1.0 + 1e-12 and M.ssim(x, y) < 1.0
    assert abs(M.ssim(x, y) - M.ssim(y, x)) <= 1e-15
    with pytest.raises(ValueError, match="11 x 11"):
        M.ssim(x[:10], y[:10])


def test_mse_and_psnr_follow_the_trainers_rule():
    import torch
    from rtx_nerf_amd.train import psnr
    x, y = _pair(12, 16, 5)
    p, t = x.astype(np.float32), y.astype(np.float32)
    mse, db = M.mse_psnr(p, t)
    assert abs(mse - float(((p.astype(np.float64) - t.astype(np.float64)) ** 2).mean())) <= 1e-18
    # train.psnr() takes a float32 torch mean: the same rule to float32's accuracy
    assert abs(db - psnr(torch.from_numpy(p), torch.from_numpy(t))) <= 1e-4
    assert M.mse_psnr(p, p) == (0.0, 120.0)                                   # the cap: 10 log10(1 / 1e-12)
    assert psnr(torch.from_numpy(p), torch.from_numpy(p)) == pytest.approx(120.0, abs=1e-9)
    tiny = p + np.float32(1e-7)
    assert M.mse_psnr(tiny, p)[1] == 120.0


def test_target_rule_u8_and_rgba_over_a_background():
    rng = np.random.default_rng(6)
    u8 = rng.integers(0, 256, (2, 5, 7, 4), dtype=np.uint8)
    t = M.target_f32(u8[..., :3].copy(), 1)
    assert t.dtype == np.float32 and np.array_equal(t, u8[1, ..., :3].astype(np.float32) / np.float32(255.0))
    bg = (0.2, 0.5, 0.9)
    t4 = M.target_f32(u8, 1, bg)
    f = u8[1].astype(np.float64) / 255.0
    want = f[..., 3:4] * f[..., :3] + (1.0 - f[..., 3:4]) * np.asarray(bg)
    assert t4.dtype == np.float32 and np.abs(t4 - want).max() <= 3e-7
    u8[1, 0, 0, 3], u8[1, 0, 1, 3] = 255, 0                                   # opaque keeps the colour, clear the background, exactly
    t4 = M.target_f32(u8, 1, bg)
    assert np.array_equal(t4[0, 0], u8[1, 0, 0, :3].astype(np.float32) / np.float32(255.0))
    assert np.array_equal(t4[0, 1], np.asarray(bg, np.float32))
    mse, db, s = M.record(t4, u8, 1, bg, with_ssim=False)
    assert (mse, db) == (0.0, 120.0) and np.isnan(s)
