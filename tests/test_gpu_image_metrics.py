"""rtxn_image_metrics on the GPU against the float64 restatement (tests/_image_metrics_float64.py), at the smallest sizes at which
the tiling can go wrong: 11 x 11 (one window), 12 x 11 and 11 x 12, 37 x 29 (partial tiles on both axes, four blocks), 64 x 48
(twelve blocks) and 283 x 281 (289 tiles: the fold's second round); every storage format; noise, a ramp, a hard edge and the
near-white pair 1 - {0, 1, 2}/255 whose variance the raw-moment form loses in fp32.

Bars.  mse: 1e-6 relative, psnr 1e-5 dB (10 / ln 10 times that).  ssim: SSIM_BAR, 10 x the largest error observed over every case
here (the table is in DESIGN 5.18; each case prints its error before it asserts), and -- fixed before anything was measured --
1e-5 on the near-white pair at 37 x 29 and 64 x 48, where the raw-moment form is off by 3.4e-5."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_metrics_float64 as M  # noqa: E402

pytestmark = pytest.mark.gpu

SSIM_BAR = 1.4e-6          # 10 x 1.40e-7, the largest error observed (11 x 11, RGBA32F over white, noise: one window)
SIZES = [(11, 11), (12, 11), (11, 12), (37, 29), (64, 48)]           # (width, height)
FORMATS = [("rgb", "u8", None), ("rgb", "f32", None), ("rgba", "u8", (1.0, 1.0, 1.0)), ("rgba", "f32", (1.0, 1.0, 1.0)),
           ("rgba", "u8", (0.2, 0.5, 0.9)), ("rgba", "f32", (0.2, 0.5, 0.9))]
KINDS = ["noise", "ramp", "edge", "near_white"]


def make_pair(kind, w, h, seed):
    """(target u8 [h, w, 3], pred float32 [h, w, 3]) of one kind"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        t = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = t / 255.0 + 0.1 * rng.standard_normal((h, w, 3))
    elif kind == "ramp":
        x, y = np.meshgrid(np.arange(w) / max(w - 1, 1), np.arange(h) / max(h - 1, 1))
        f = np.stack([x, y, 0.5 * (x + y)], -1)
        t = np.rint(255.0 * f).astype(np.uint8)
        p = 0.9 * f + 0.05
    elif kind == "edge":
        t = np.full((h, w, 3), 26, np.uint8)
        t[:, w // 2:] = 255
        p = np.full((h, w, 3), 0.1)
        p[:, w // 2 + 1:] = 1.0                       # the edge one pixel to the right
    elif kind == "near_white":
        t = (255 - rng.integers(0, 3, (h, w, 3))).astype(np.uint8)
        p = 1.0 - rng.integers(0, 3, (h, w, 3)) / 255.0
    else:
        raise ValueError(kind)
    return t, p.astype(np.float32)


def make_set(t_u8, layout, storage, seed):
    """3 frames [3, h, w, C] with the target as frame 1 and noise around it; rgba: a random alpha on every frame"""
    rng = np.random.default_rng(seed + 1000)
    h, w, _ = t_u8.shape
    c = 4 if layout == "rgba" else 3
    frames = rng.integers(0, 256, (3, h, w, c), dtype=np.uint8)
    frames[1, ..., :3] = t_u8
    if storage == "f32":
        return frames.astype(np.float32) / np.float32(255.0)
    return frames


def run(gpu, frames, pred, background=None, image=1, **kw):
    """the record of frame `image` as a numpy float64 [3]"""
    from rtx_nerf_amd import api
    n = frames.shape[0]
    s = api.ImageSet(gpu.from_numpy(frames).cuda(), gpu.zeros((n, 16), device="cuda"), 2.0)
    rec = api.image_metrics(s, image, gpu.from_numpy(np.ascontiguousarray(pred)).cuda(), background=background, **kw)
    return rec.cpu().numpy()


def bits(rec):
    return np.asarray(rec, np.float64).view(np.int64)


def check_case(gpu, kind, w, h, layout, storage, bg, seed):
    t, p = make_pair(kind, w, h, seed)
    frames = make_set(t, layout, storage, seed)
    got = run(gpu, frames, p, bg)
    want = M.record(p, frames, 1, bg)
    err_mse = abs(got[0] - want[0]) / want[0]
    err_db = abs(got[1] - want[1])
    err_ssim = abs(got[2] - want[2])
    print(f"image_metrics {w}x{h} {layout}/{storage} bg={bg} {kind}: mse rel {err_mse:.2e} psnr {err_db:.2e} dB ssim abs {err_ssim:.2e} "
          f"(ssim {want[2]:.6f})")
    return err_mse, err_db, err_ssim


@pytest.mark.parametrize("w,h", SIZES)
def test_record_against_float64(gpu, w, h):
    worst = [0.0, 0.0, 0.0]
    failures = []
    for fi, (layout, storage, bg) in enumerate(FORMATS):
        for ki, kind in enumerate(KINDS):
            e = check_case(gpu, kind, w, h, layout, storage, bg, seed=100 * fi + ki)
            worst = [max(a, b) for a, b in zip(worst, e)]
            if e[0] > 1e-6 or e[1] > 1e-5 or e[2] > SSIM_BAR:
                failures.append((layout, storage, bg, kind, e))
            if kind == "near_white" and (w, h) in ((37, 29), (64, 48)) and e[2] > 1e-5:
                failures.append(("near-white bar", layout, storage, bg, e))
    print(f"image_metrics {w}x{h}: worst mse rel {worst[0]:.2e}, psnr {worst[1]:.2e} dB, ssim abs {worst[2]:.2e}")
    assert not failures, failures


def test_the_fold_takes_more_partials_than_it_has_threads(gpu):
    """283 x 281: 17 x 17 = 289 tiles, so thread 0 .. 32 of the fold take two partials each"""
    e = check_case(gpu, "noise", 283, 281, "rgb", "u8", None, seed=7)
    e2 = check_case(gpu, "near_white", 283, 281, "rgba", "u8", (1.0, 1.0, 1.0), seed=8)
    assert max(e[0], e2[0]) <= 1e-6 and max(e[1], e2[1]) <= 1e-5 and e[2] <= SSIM_BAR and e2[2] <= min(SSIM_BAR, 1e-5)


@pytest.mark.parametrize("layout,storage,bg", [("rgb", "u8", None), ("rgb", "f32", None), ("rgba", "u8", (1.0, 1.0, 1.0)),
                                               ("rgba", "f32", (0.2, 0.5, 0.9))])
def test_identical_images(gpu, layout, storage, bg):
    t, _ = make_pair("noise", 37, 29, 11)
    frames = make_set(t, layout, storage, 11)
    got = run(gpu, frames, M.target_f32(frames, 1, bg), bg)
    print(f"image_metrics identical {layout}/{storage}: {got.tolist()}, 1 - ssim = {1.0 - got[2]:.2e}")
    assert got[0] == 0.0 and got[1] == 120.0 and abs(1.0 - got[2]) <= 1e-6


@pytest.mark.parametrize("a,b_u8", [(0.3, 179), (1.0, 0), (0.5, 128), (1.0, 255)])
def test_constant_images_closed_form(gpu, a, b_u8):
    w, h = 37, 29
    frames = np.full((3, h, w, 3), b_u8, np.uint8)
    got = run(gpu, frames, np.full((h, w, 3), a, np.float32))
    af, bf = float(np.float32(a)), float(np.float32(b_u8) / np.float32(255.0))
    want = (2 * af * bf + M.C1) / (af * af + bf * bf + M.C1)
    print(f"image_metrics constant {a} vs {b_u8}/255: ssim {got[2]:.9f}, closed form {want:.9f}, error {abs(got[2] - want):.2e}")
    assert abs(got[2] - want) <= SSIM_BAR
    assert abs(got[0] - (af - bf) ** 2) <= 1e-6 * (af - bf) ** 2


def test_clamp_scores_the_clamped_copy_bit_for_bit(gpu):
    t, p = make_pair("noise", 37, 29, 21)             # noise of 0.1 around k/255: values below 0 and above 1
    assert p.min() < 0.0 and p.max() > 1.0
    frames = make_set(t, "rgba", "u8", 21)
    bg = (0.2, 0.5, 0.9)
    clamped = run(gpu, frames, p, bg, clamp=True)
    copy = run(gpu, frames, np.clip(p, np.float32(0.0), np.float32(1.0)), bg)
    plain = run(gpu, frames, p, bg)
    assert np.array_equal(bits(clamped), bits(copy))
    assert plain[0] > clamped[0]
    want = M.record(p, frames, 1, bg, clamp=True)
    assert abs(clamped[0] - want[0]) <= 1e-6 * want[0] and abs(clamped[2] - want[2]) <= SSIM_BAR


def test_without_the_ssim_flag(gpu):
    from rtx_nerf_amd import _lib
    for w, h in ((37, 29), (64, 48)):
        t, p = make_pair("noise", w, h, 31)
        frames = make_set(t, "rgb", "u8", 31)
        full, bare = run(gpu, frames, p), run(gpu, frames, p, ssim=False)
        assert np.isnan(bare[2]) and not np.isnan(full[2])
        assert np.array_equal(bits(full[:2]), bits(bare[:2]))
    t, p = make_pair("noise", 5, 7, 32)               # smaller than a window: accepted without the flag, refused with it
    frames = make_set(t, "rgba", "f32", 32)
    got = run(gpu, frames, p, (1.0, 1.0, 1.0), ssim=False)
    want = M.record(p, frames, 1, (1.0, 1.0, 1.0), with_ssim=False)
    assert abs(got[0] - want[0]) <= 1e-6 * want[0] and abs(got[1] - want[1]) <= 1e-5 and np.isnan(got[2])
    with pytest.raises(_lib.RtxnError, match="at least 11 x 11, not 5 x 7"):
        run(gpu, frames, p, (1.0, 1.0, 1.0))


@pytest.mark.parametrize("w,h", [(37, 29), (64, 48)])
def test_two_runs_give_identical_bits(gpu, w, h):
    t, p = make_pair("noise", w, h, 41)
    frames = make_set(t, "rgba", "u8", 41)
    a, b = run(gpu, frames, p, (0.2, 0.5, 0.9)), run(gpu, frames, p, (0.2, 0.5, 0.9))
    assert np.array_equal(bits(a), bits(b)) and not np.isnan(a).any()


def test_record_of_one_frame_ignores_its_neighbours(gpu):
    t, p = make_pair("ramp", 37, 29, 51)
    for storage in ("u8", "f32"):
        frames = make_set(t, "rgb", storage, 51)
        other = frames.copy()
        other[0], other[2] = 0, frames[0]
        a, b = run(gpu, frames, p), run(gpu, other, p)
        assert np.array_equal(bits(a), bits(b))
        assert not np.array_equal(bits(a), bits(run(gpu, frames, p, image=0)))


def test_nothing_is_written_outside_the_workspace_and_the_record(gpu):
    from rtx_nerf_amd import api
    torch = gpu
    w, h = 64, 48
    t, p = make_pair("noise", w, h, 61)
    frames = make_set(t, "rgb", "u8", 61)
    s = api.ImageSet(torch.from_numpy(frames).cuda(), torch.zeros((3, 16), device="cuda"), 2.0)
    need = api.image_metrics_workspace_bytes(w, h)
    assert need == 192 and api.image_metrics_workspace(s).numel() == need
    big = torch.full((need + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    recs = torch.full((5,), -7.0, dtype=torch.float64, device="cuda")
    pred = torch.from_numpy(p).cuda()
    api.image_metrics(s, 1, pred, record=recs[1:4], workspace=big[64:64 + need])
    torch.cuda.synchronize()
    assert bool((big[:64] == 0xA5).all()) and bool((big[64 + need:] == 0xA5).all())
    assert not bool((big[64:64 + need] == 0xA5).all())
    assert recs[0].item() == -7.0 and recs[4].item() == -7.0
    assert np.array_equal(bits(recs[1:4].cpu().numpy()), bits(run(gpu, frames, p)))
