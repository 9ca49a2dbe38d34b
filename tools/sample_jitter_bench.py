#!/usr/bin/env python3
"""What the sample jitter costs and buys.
Cost: the whole eager step, midpoints vs Trainer(sample_jitter=True), on the configs[2] batch (4096 rays, hash grid + 4x64 MLP,
128^3 stand-in occupancy) and the reference-model batch (22,528 rays, Composite-Frequency + 8x128 MLP); the two variants are
separate trainers from the same seed, run in alternation, timed with HIP events around back-to-back steps.
Convergence: the demo scene of examples/train_synthetic.py (--make-demo) trained both ways from the same seed and batches,
held-out PSNR at fixed step counts.
  python tools/sample_jitter_bench.py [--reps 5] [--steps 10] [--train-steps 800] [--skip-cost] [--skip-convergence]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np
import torch

from rtx_nerf_amd import loader, scenes
from rtx_nerf_amd.train import RayDataset, Trainer, camera_rays, psnr
from train_demo import teacher_field

CONFIGS = {"configs[2] 4096 rays, hash + 4x64": dict(batch=4096, encoding="hash", neurons=64, layers=4, n_dir_freqs=4),
           "reference model 22528 rays, freq + 8x128": dict(batch=22528, encoding="freq", neurons=128, layers=8, n_dir_freqs=12)}
VARIANTS = {"midpoint": dict(), "jitter": dict(sample_jitter=True, jitter_seed=9)}


def cost(a):
    R = 128
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(R, seed=0)).view(np.int32).copy()).cuda()
    focal = scenes.lego_focal_length(True)
    for cname, c in CONFIGS.items():
        B = c["batch"]
        trs = {v: Trainer(R, occ, encoding=c["encoding"], n_neurons=c["neurons"], n_hidden_layers=c["layers"],
                          hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                          n_dir_freqs=c["n_dir_freqs"], batch_rays=max(B, 128 * 128), max_segments=max(B, 128 * 128) * 10, lr=1e-2,
                          loss_scale=128.0, density_scale=300.0, mode="nerf", **kw) for v, kw in VARIANTS.items()}
        t0 = trs["midpoint"]
        ro, rd, tg = [], [], []
        for i in range(8):
            o, d = camera_rays(scenes.pose_spherical(45.0 * i + 15.0, -30.0, origin_scale=10.0), focal, 128, 128)
            ro.append(o); rd.append(d)
            tg.append(t0.render_rays(o, d, radiance_fn=teacher_field).clone())
        ro, rd, tg = torch.cat(ro), torch.cat(rd), torch.cat(tg)
        g = torch.Generator(device="cuda").manual_seed(42)
        batches = []
        for _ in range(a.steps):
            idx = torch.randint(0, ro.shape[0], (B,), device="cuda", generator=g)
            batches.append((ro[idx].contiguous(), rd[idx].contiguous(), tg[idx].contiguous()))
        for tr in trs.values():                       # warm-up
            for b in batches[:3]:
                tr.step(*b)
        torch.cuda.synchronize()
        res = {v: [] for v in VARIANTS}
        for _ in range(a.reps):
            for v, tr in trs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for b in batches:
                    tr.step(*b)
                e1.record()
                torch.cuda.synchronize()
                res[v].append(e0.elapsed_time(e1) / len(batches))
        out = {v: {"step_ms_median": round(float(np.median(r)), 3), "step_ms_reps": [round(x, 3) for x in r]} for v, r in res.items()}
        print(json.dumps({"config": cname, "segments_last_step": int(t0.total.item()), "variants": out}), flush=True)
        del trs
        torch.cuda.empty_cache()


def convergence(a):
    from train_synthetic import make_demo
    at = sorted({s for s in (100, 200, 400, 800, 1600, 3200) if s <= a.train_steps} | {a.train_steps})
    with tempfile.TemporaryDirectory() as path:
        make_demo(path)
        ds = loader.load_images_json(path, "train", flags=2)
    n_hold = max(1, ds.images.shape[0] // 8)
    train_ds = loader.ImageDataset(ds.images[:-n_hold], ds.poses[:-n_hold], ds.focal, ds.image_width, ds.image_height, 3, ds.camera_angle_x)
    rays, focal = RayDataset.from_images(train_ds, origin_scale=0.1)
    W, H, R, B = ds.image_width, ds.image_height, 32, 4096
    held = [(camera_rays(ds.poses[-1 - k], focal, W, H, origin_scale=0.1), torch.from_numpy(ds.images[-1 - k].reshape(-1, 3)).cuda())
            for k in range(n_hold)]
    for encoding in ("hash", "freq"):
        out = {}
        for v, kw in VARIANTS.items():
            tr = Trainer(R, None, encoding=encoding, n_neurons=64, n_hidden_layers=2 if encoding == "hash" else 4,
                         hashgrid=dict(n_levels=8, n_features=2, log2_hashmap_size=15, base_resolution=8, per_level_scale=1.5),
                         batch_rays=max(B, W * H), max_segments=max(B, W * H) * (3 * R), lr=1e-2 if encoding == "hash" else 2e-3,
                         density_scale=150.0, **kw)
            g = torch.Generator(device="cuda").manual_seed(0)
            curve = {}
            for it in range(a.train_steps):
                tr.step(*rays.sample_batch(B, g))
                if (it + 1) % 100 == 0 and it + 1 >= 200:
                    tr.update_occupancy(threshold=0.01)
                if it + 1 in at:
                    curve[it + 1] = round(float(np.mean([psnr(tr.render_rays(o, d), gt) for (o, d), gt in held])), 2)
            out[v] = curve
        print(json.dumps({"scene": f"demo {W}x{H}, {train_ds.images.shape[0]} training frames, {n_hold} held out", "encoding": encoding,
                          "held_out_psnr_db": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--train-steps", type=int, default=800)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-convergence", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if not a.skip_cost:
        cost(a)
    if not a.skip_convergence:
        convergence(a)


if __name__ == "__main__":
    main()
