#!/usr/bin/env python3
"""A/B of training over a background: the training compositor kernel and the whole eager step, plain (black) vs
CONSTANT (white, 3-channel targets composited over white) vs RANDOM + RGBA, on the configs[2] batch (4096 rays, hash grid +
4x64 MLP, 128^3 stand-in occupancy) and the reference-model batch (22,528 rays, Composite-Frequency + 8x128 MLP).  The three
variants are separate trainers from the same seed, run in alternation; times are HIP events (Trainer.time_stages for the
compositor stage, back-to-back steps for the step).  The live-segment fraction is printed beside them: the backward's cost
follows it.
  python tools/train_background_bench.py [--reps 3] [--steps 10]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from rtx_nerf_amd import scenes
from rtx_nerf_amd.train import Trainer, camera_rays
from train_demo import teacher_field

CONFIGS = {"configs[2] 4096 rays, hash + 4x64": dict(batch=4096, encoding="hash", neurons=64, layers=4),
           "reference model 22528 rays, freq + 8x128": dict(batch=22528, encoding="freq", neurons=128, layers=8)}
VARIANTS = {"plain": dict(), "constant": dict(background=(1.0, 1.0, 1.0)), "random+rgba": dict(background="random")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = 128
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(R, seed=0)).view(np.int32).copy()).cuda()
    focal = scenes.lego_focal_length(True)
    for cname, c in CONFIGS.items():
        B = c["batch"]
        trs = {v: Trainer(R, occ, encoding=c["encoding"], n_neurons=c["neurons"], n_hidden_layers=c["layers"],
                          hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                          n_dir_freqs=4, batch_rays=max(B, 128 * 128), max_segments=max(B, 128 * 128) * 10, lr=1e-2,
                          loss_scale=128.0, density_scale=300.0,
                          mode="nerf", **kw) for v, kw in VARIANTS.items()}
        t0 = trs["plain"]
        ro, rd, black, white = [], [], [], []
        for i in range(8):
            o, d = camera_rays(scenes.pose_spherical(45.0 * i + 15.0, -30.0, origin_scale=10.0), focal, 128, 128)
            ro.append(o); rd.append(d)
            black.append(t0.render_rays(o, d, radiance_fn=teacher_field).clone())
            white.append(t0.render_rays(o, d, radiance_fn=teacher_field, background=(1.0, 1.0, 1.0)).clone())
        ro, rd, black, white = torch.cat(ro), torch.cat(rd), torch.cat(black), torch.cat(white)
        alpha = (1.0 - (white - black).mean(1, keepdim=True)).clamp(0, 1)
        rgba = torch.cat([torch.where(alpha > 1e-6, black / alpha.clamp_min(1e-6), torch.zeros_like(black)), alpha], 1)
        targets = {"plain": black, "constant": white, "random+rgba": rgba}
        g = torch.Generator(device="cuda").manual_seed(42)
        res = {v: {"composite_ms": [], "step_ms": [], "live": []} for v in VARIANTS}
        batches = []
        for _ in range(a.steps):
            idx = torch.randint(0, ro.shape[0], (B,), device="cuda", generator=g)
            batches.append((ro[idx].contiguous(), rd[idx].contiguous(), idx))
        for v, tr in trs.items():                     # warm-up
            for o, d, idx in batches[:3]:
                tr.step(o, d, targets[v][idx].contiguous())
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for v, tr in trs.items():
                comp = []
                for o, d, idx in batches:
                    st = tr.time_stages(o, d, targets[v][idx].contiguous(), steps=1)
                    comp.append(st["composite_fwd+l2+bwd"])
                    res[v]["live"].append(int(tr.live_ws[0].item()) / max(1, int(tr.total.item())))
                res[v]["composite_ms"].append(float(np.median(comp)))
                tg = [targets[v][idx].contiguous() for _, _, idx in batches]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for (o, d, _), t in zip(batches, tg):
                    tr.step(o, d, t)
                e1.record()
                torch.cuda.synchronize()
                res[v]["step_ms"].append(e0.elapsed_time(e1) / len(batches))
        out = {v: {"composite_ms_median": round(float(np.median(r["composite_ms"])), 4),
                   "composite_ms_reps": [round(x, 4) for x in r["composite_ms"]],
                   "step_ms_median": round(float(np.median(r["step_ms"])), 3), "step_ms_reps": [round(x, 3) for x in r["step_ms"]],
                   "live_fraction_mean": round(float(np.mean(r["live"])), 4)} for v, r in res.items()}
        print(json.dumps({"config": cname, "segments_last_step": int(t0.total.item()), "variants": out}), flush=True)
        del trs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
