#!/usr/bin/env python3
"""What drawing the batch on the device costs and saves.  One JSON line: the HBM bytes the two datasets hold, and
ms per step of three rows on the configs[2]-shaped trainer (4096 rays, hash grid + 4x64 MLP, 128^3 stand-in occupancy):
  (a) ray_dataset   RayDataset.sample_batch (torch.randint + three gathers) -> copies into graph_rays_o / _d / graph_targets ->
                    step_captured(): the loop without rtxn_draw_batch;
  (b) device_draw   capture_step(draw=True): step_captured() alone, the draw is the graph's first node;
  (c) draw_alone    api.draw_batch by itself (launch + kernel), uint8 and float frames.
(a) and (b) are separate trainers from the same seed over the same frames; the rows run in alternation, `reps` times `steps`
back-to-back steps each between HIP events, and the line carries every repetition, the medians, and the spread of the paired
differences (b) - (a), which is what a claim about the two has to clear.
  python tools/draw_batch_bench.py [--reps 7] [--steps 200] [--frames 8] [--res 128]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from rtx_nerf_amd import api, loader, scenes
from rtx_nerf_amd.train import RayDataset, Trainer, camera_rays
from train_demo import teacher_field

B = 4096


def trainer(occ, res):
    return Trainer(128, occ, encoding="hash", n_neurons=64, n_hidden_layers=4,
                   hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                   n_dir_freqs=4, batch_rays=max(B, res * res), max_segments=max(B, res * res) * 10, lr=1e-2, loss_scale=128.0,
                   density_scale=300.0, mode="nerf")


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--res", type=int, default=128)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = a.res
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(128, seed=0)).view(np.int32).copy()).cuda()
    focal = scenes.lego_focal_length(True)
    ta, tb = trainer(occ, res), trainer(occ, res)
    poses, frames = [], []
    for i in range(a.frames):
        pose = scenes.pose_spherical(360.0 * i / a.frames + 15.0, -30.0, origin_scale=10.0)
        o, d = camera_rays(pose, focal, res, res)
        frames.append(ta.render_rays(o, d, radiance_fn=teacher_field).reshape(res, res, 3).clamp(0, 1).cpu().numpy())
        poses.append(np.asarray(pose, np.float32))
    ds = loader.ImageDataset(np.stack(frames), np.stack(poses), 0.0, res, res, 3, scenes.LEGO_CAMERA_ANGLE_X)
    rays, _ = RayDataset.from_images(ds)
    set_u8, _ = api.ImageSet.from_dataset(ds, storage="u8")
    set_f32, _ = api.ImageSet.from_dataset(ds, storage="f32")
    g = torch.Generator(device="cuda").manual_seed(0)
    cap = ta.max_segments
    ta.capture_step(B, launch_segments=cap)
    tb.attach_images(set_u8)
    tb.capture_step(B, launch_segments=cap, draw=True)
    o, d, t = (torch.empty((B, 3), device="cuda") for _ in range(3))
    step = torch.zeros(1, dtype=torch.int32, device="cuda")

    def row_a():
        ro, rd, px = rays.sample_batch(B, g)
        ta.graph_rays_o.copy_(ro); ta.graph_rays_d.copy_(rd); ta.graph_targets.copy_(px)
        ta.step_captured()

    rows = {"ray_dataset": row_a, "device_draw": tb.step_captured,
            "draw_alone_u8": lambda: api.draw_batch(set_u8, B, 0, step, o, d, t),
            "draw_alone_f32": lambda: api.draw_batch(set_f32, B, 0, step, o, d, t)}
    for fn in rows.values():                       # warm-up: every shape the timed windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, fn in rows.items():
            ms[k].append(timed(fn, a.steps))
    diff = [y - x for x, y in zip(ms["ray_dataset"], ms["device_draw"])]
    out = {"rays": B, "frames": f"{a.frames} x {res}x{res} RGB", "reps": a.reps, "steps_per_rep": a.steps,
           "hbm_bytes": {"ray_dataset": int(sum(x.numel() * x.element_size() for x in (rays.rays_o, rays.rays_d, rays.pixels))),
                         "image_set_u8": set_u8.nbytes(), "image_set_f32": set_f32.nbytes()},
           "ms_per_step": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
           "device_draw_minus_ray_dataset_ms": {"median": round(float(np.median(diff)), 4), "min": round(min(diff), 4),
                                                "max": round(max(diff), 4)},
           "segments_last_step": int(tb.total.item()), "truncated_steps": [ta.truncated_steps, tb.truncated_steps]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
