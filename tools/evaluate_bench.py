#!/usr/bin/env python3
"""What scoring a held-out frame on the device costs.  One JSON line, ms per frame on the configs[2]-shaped trainer
(hash grid + 4x64 MLP, 128^3 stand-in occupancy) over `frames` poses at res x res:
  (a) render          the bare frame: the evaluation pipeline's render() with the pose read from the image set;
  (b) evaluate        Trainer.evaluate(): (a) + one rtxn_image_metrics per frame, nothing read on the host;
  (c) host_psnr       the route it replaces: (a), then train.psnr() against a device target -- a torch mean and a host float per frame;
  (d) metrics_alone   rtxn_image_metrics by itself (two launches) at res x res and at the demo scene's 64 x 64, RGB8 and RGBA32F
                      targets, with and without SSIM.
The frames are noise (the kernels' time does not depend on the values).  The rows run in alternation, `reps` times, each over
`steps` frames between HIP events; the line carries every repetition, the medians, and the spread of the paired differences
(b) - (a), which is what a claim about the metrics' share of a frame has to clear.
  python tools/evaluate_bench.py [--reps 7] [--steps 40] [--frames 4] [--res 800]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from rtx_nerf_amd import api, scenes
from rtx_nerf_amd.train import Trainer, psnr


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def noise_set(n, res, channels, storage, poses, focal, seed=0):
    img = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, res, res, channels), dtype=np.uint8)).cuda()
    if storage == "f32":
        img = img.float() / 255.0
    return api.ImageSet(img, poses, focal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--res", type=int, default=800)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res, n = a.res, a.frames
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(128, seed=0)).view(np.int32).copy()).cuda()
    focal = scenes.lego_focal_length(True)
    tr = Trainer(128, occ, encoding="hash", n_neurons=64, n_hidden_layers=4,
                 hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                 n_dir_freqs=4, batch_rays=4096, max_segments=4096 * 10, lr=1e-2, loss_scale=128.0, density_scale=300.0, mode="nerf")
    poses = torch.from_numpy(np.stack([np.asarray(scenes.pose_spherical(360.0 * i / n + 15.0, -30.0, origin_scale=10.0), np.float32)
                                       for i in range(n)])).cuda()
    held = noise_set(n, res, 3, "u8", poses, focal)
    rec = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    tr.evaluate(held, out=rec)                                  # builds and calibrates the pipeline
    pipe = next(iter(tr._eval_pipelines.values()))[0]
    gt = [held.images[i].reshape(-1, 3).float() / 255.0 for i in range(n)]
    frame = [0]

    def row_render():
        pipe.render(look_at=held.poses[frame[0] % n])
        frame[0] += 1

    def row_host():
        i = frame[0] % n
        psnr(pipe.render(look_at=held.poses[i]), gt[i])
        frame[0] += 1

    rows = {"render": (row_render, 1), "evaluate": (lambda: tr.evaluate(held, out=rec), n), "host_psnr": (row_host, 1)}
    for size in sorted({res, 64}):
        for channels, storage in ((3, "u8"), (4, "f32")):
            s = noise_set(1, size, channels, storage, poses[:1], focal, seed=1)
            pred = torch.rand((size * size, 3), device="cuda")
            ws, r1 = api.image_metrics_workspace(s), torch.empty(3, dtype=torch.float64, device="cuda")
            for ssim in (True, False):
                name = f"metrics_alone_{size}x{size}_{'rgb' if channels == 3 else 'rgba'}_{storage}_{'ssim' if ssim else 'mse_only'}"
                rows[name] = (lambda s=s, pred=pred, ws=ws, r1=r1, ssim=ssim: api.image_metrics(
                    s, 0, pred, background=(1.0, 1.0, 1.0), ssim=ssim, record=r1, workspace=ws), 1)
    for fn, _ in rows.values():                                 # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, (fn, per) in rows.items():
            calls = max(1, a.steps // per) if not k.startswith("metrics_alone") else 10 * a.steps
            ms[k].append(timed(fn, calls) / per)
    diff = [y - x for x, y in zip(ms["render"], ms["evaluate"])]
    out = {"frames": f"{n} x {res}x{res} RGB8", "reps": a.reps, "frames_per_rep": a.steps, "segments_last_frame": int(pipe.total.item()),
           "overflowed": bool(pipe.overflowed()), "psnr_mean_db": round(float(rec[:, 1].mean()), 3),
           "ssim_mean": round(float(rec[:, 2].mean()), 5),
           "ms_per_frame": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
           "evaluate_minus_render_ms": {"median": round(float(np.median(diff)), 4), "min": round(min(diff), 4), "max": round(max(diff), 4)}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
