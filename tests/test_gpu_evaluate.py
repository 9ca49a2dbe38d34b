"""Trainer.evaluate on the GPU: a small trainer (grid 16, a four-level hash grid, or the frequency model) and an ImageSet of
three 24 x 20 frames.  A row of evaluate() is, bit for bit, api.image_metrics of the frame render_pipeline() draws at that
frame's pose; its mse is the float64 mean of squares of that frame against the target; the rows follow `images`; weights="ema"
scores the averaged model; a captured evaluate() follows the weights."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_metrics_float64 as M  # noqa: E402

pytestmark = pytest.mark.gpu

R, B, W, H = 16, 900, 24, 20
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
BG = (0.2, 0.5, 0.9)


def _trainer(torch, encoding="hash", **kw):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()
    neurons, layers = (64, 4) if encoding == "hash" else (128, 8)
    return Trainer(R, occ, encoding=encoding, n_neurons=neurons, n_hidden_layers=layers, hashgrid=HGD if encoding == "hash" else None,
                   n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2, loss_scale=128.0, density_scale=120.0, mode="nerf", seed=3,
                   **kw)


def _train(torch, tr, steps):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    for i in range(steps):
        o, d = camera_rays(scenes.pose_spherical(40.0 + 50.0 * i, -30.0 + 5.0 * i, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
        t = torch.from_numpy(np.random.default_rng(i).uniform(0, 1, (B, tr.target_channels)).astype(np.float32)).cuda()
        tr.step(o, d, t)


def _image_set(torch, layout, storage):
    """(ImageSet, its frames as numpy): three frames of noise at 24 x 20, poses around the grid"""
    from rtx_nerf_amd import api, scenes
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (3, H, W, 4 if layout == "rgba" else 3), dtype=np.uint8)
    if storage == "f32":
        frames = frames.astype(np.float32) / np.float32(255.0)
    poses = np.stack([scenes.pose_spherical(30.0 + 70.0 * i, -25.0 - 10.0 * i, origin_scale=10.0) for i in range(3)]).astype(np.float32)
    s = api.ImageSet(torch.from_numpy(frames).cuda(), torch.from_numpy(poses).cuda(), scenes.lego_focal_length(True))
    return s, frames


def _bits(t):
    """the bit patterns of a float64 tensor"""
    return t.detach().cpu().contiguous().numpy().view(np.int64)


def _frames_and_rows(torch, tr, s, bg, weights="live"):
    """per frame of the set: what a pipeline of render_pipeline() draws at its pose, and api.image_metrics of it"""
    from rtx_nerf_amd import api
    pipe = tr.render_pipeline(W, H, s.focal_length, max_segments=W * H * 40, weights=weights)
    frames, rows = [], []
    for i in range(s.n_images):
        pipe.set_pose(s.poses[i])
        frame = pipe.render_ex(background=bg, depth=False, opacity=False)[0] if bg is not None else pipe.render()
        frames.append(frame.clone())
        rows.append(api.image_metrics(s, i, frames[-1], background=bg))
    torch.cuda.synchronize()
    assert not pipe.overflowed()
    return frames, torch.stack(rows)


@pytest.mark.parametrize("encoding,layout,storage,bg", [("hash", "rgb", "u8", None), ("hash", "rgba", "f32", BG), ("freq", "rgb", "u8", None)])
def test_rows_are_the_metrics_of_the_pipelines_frames(gpu, encoding, layout, storage, bg):
    torch = gpu
    tr = _trainer(torch, encoding, **(dict(background=bg, target_channels=4) if bg is not None else {}))
    _train(torch, tr, 3)                                      # the frequency model's inference packing is stale now: evaluate() syncs it
    s, frames_np = _image_set(torch, layout, storage)
    rec = tr.evaluate(s)                                      # an RGBA set takes the trainer's constant background
    assert rec.shape == (3, 3) and rec.dtype == torch.float64 and rec.is_cuda
    frames, rows = _frames_and_rows(torch, tr, s, bg)
    assert np.array_equal(_bits(rec), _bits(rows)), (rec, rows)
    assert bool(torch.isfinite(rec).all()) and float(frames[0].abs().max()) > 0
    for i in range(3):
        target = torch.from_numpy(M.target_f32(frames_np, i, bg)).cuda().double().reshape(-1, 3)
        mse = float(((frames[i].double() - target) ** 2).mean())
        assert abs(float(rec[i, 0]) - mse) <= 1e-6 * mse
        assert abs(float(rec[i, 1]) - 10.0 * np.log10(1.0 / mse)) <= 1e-5
    picked = tr.evaluate(s, images=[2, 0])
    assert np.array_equal(_bits(picked), _bits(rec[[2, 0]]))
    again = tr.evaluate(s, background=bg, out=torch.empty((3, 3), dtype=torch.float64, device="cuda"))
    assert np.array_equal(_bits(again), _bits(rec))
    assert len(tr._eval_pipelines) == 1                       # one cached pipeline for the three calls
    bare = tr.evaluate(s, images=[1], ssim=False)
    assert np.array_equal(_bits(bare[0, :2]), _bits(rec[1, :2])) and bool(torch.isnan(bare[0, 2]))


def test_an_explicit_background_under_a_trainer_without_one(gpu):
    torch = gpu
    tr = _trainer(torch)
    s, _ = _image_set(torch, "rgba", "u8")
    with pytest.raises(ValueError, match="4-channel image set needs a colour"):
        tr.evaluate(s)
    rec = tr.evaluate(s, background=BG)
    _, rows = _frames_and_rows(torch, tr, s, BG)
    assert np.array_equal(_bits(rec), _bits(rows))
    white = tr.evaluate(s, background=(1.0, 1.0, 1.0))
    assert not np.array_equal(_bits(white), _bits(rec))


def test_ema_rows_score_the_averaged_model(gpu):
    torch = gpu
    tr = _trainer(torch, ema_decay=0.9)
    _train(torch, tr, 10)
    s, _ = _image_set(torch, "rgb", "u8")
    live = tr.evaluate(s).clone()
    ema = tr.evaluate(s, weights="ema").clone()
    tr.sync_ema()
    _, rows = _frames_and_rows(torch, tr, s, None, weights="ema")
    assert np.array_equal(_bits(ema), _bits(rows))
    assert not np.array_equal(_bits(ema[:, 0]), _bits(live[:, 0]))
    assert np.array_equal(_bits(tr.evaluate(s)), _bits(live))              # scoring the average left the live rows alone
    with pytest.raises(RuntimeError, match="without ema_decay"):
        _trainer(torch).evaluate(s, weights="ema")


def test_a_captured_evaluate_follows_the_weights(gpu):
    torch = gpu
    tr = _trainer(torch)
    _train(torch, tr, 2)
    s, _ = _image_set(torch, "rgb", "u8")
    before = tr.evaluate(s).clone()                           # the first call: builds and calibrates the pipeline
    out = torch.zeros((3, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.evaluate(s, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(before))
    _train(torch, tr, 1)
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = tr.evaluate(s)
    assert np.array_equal(_bits(replayed), _bits(eager))
    assert not np.array_equal(_bits(replayed[:, 0]), _bits(before[:, 0]))
