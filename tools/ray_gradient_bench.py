#!/usr/bin/env python3
"""What the ray gradients and the pose refinement cost.  One JSON line: ms per step of four rows on the
configs[2]-shaped trainer (4096 rays, hash grid + 4x64 MLP, 128^3 stand-in occupancy, 8 frames of 128 x 128 drawn on the device):
  (a) plain         capture_step(draw=True): step_captured() of a trainer built without the feature -- the graph as it was;
  (b) ray_gradients the same with Trainer(ray_gradients=True): the gather and the per-ray reduction behind the scatter;
  (c) refine_poses  the same with attach_images(refine_poses=True): the pose gradient and the pose step behind the optimizer;
  (d) gather_alone  api.hashgrid_input_gradient_segments by itself over trainer (b)'s last batch (its dencT and live list).
Separate trainers from the same seed over the same frames; the rows run in alternation, `reps` times `steps` back-to-back steps
each between HIP events; the line carries every repetition, the medians and the spread of the paired differences against (a).
Beside them: time_stages() of trainer (b) -- the gather (ray_grad) next to the encoder and the scatter (hash_bwd), which move the
same table lines -- and the share of the batch's segments that are live.
  python tools/ray_gradient_bench.py [--reps 7] [--steps 200] [--frames 8] [--res 128]"""
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
from rtx_nerf_amd.train import Trainer, camera_rays
from train_demo import teacher_field

B = 4096


def trainer(occ, **kw):
    return Trainer(128, occ, encoding="hash", n_neurons=64, n_hidden_layers=4,
                   hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                   n_dir_freqs=4, batch_rays=128 * 128, max_segments=128 * 128 * 10, lr=1e-2, loss_scale=128.0,
                   density_scale=300.0, mode="nerf", **kw)


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
    ta, tb, tc = trainer(occ), trainer(occ, ray_gradients=True), trainer(occ, ray_gradients=True)
    poses, frames = [], []
    for i in range(a.frames):
        pose = scenes.pose_spherical(360.0 * i / a.frames + 15.0, -30.0, origin_scale=10.0)
        o, d = camera_rays(pose, focal, res, res)
        frames.append(ta.render_rays(o, d, radiance_fn=teacher_field).reshape(res, res, 3).clamp(0, 1).cpu().numpy())
        poses.append(np.asarray(pose, np.float32))
    ds = loader.ImageDataset(np.stack(frames), np.stack(poses), 0.0, res, res, 3, scenes.LEGO_CAMERA_ANGLE_X)
    cap = ta.max_segments
    for tr, refine in ((ta, None), (tb, None), (tc, True)):        # a set each: the refinement rewrites its poses in place
        tr.attach_images(api.ImageSet.from_dataset(ds, storage="u8")[0], refine_poses=refine)
        tr.capture_step(B, launch_segments=cap, draw=True)

    def gather_alone():
        tb._ray_gradients(cap, B, None)       # the launch the graph makes: the capacity's row stride, the live list's count

    rows = {"plain": ta.step_captured, "ray_gradients": tb.step_captured, "refine_poses": tc.step_captured}
    for fn in rows.values():                       # warm-up: every shape the timed windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    segments = tb.total.item()
    rows["gather_alone"] = gather_alone
    for _ in range(20):
        gather_alone()
    ms = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, fn in rows.items():
            ms[k].append(timed(fn, a.steps))
    live = int(tb.live_ws.view(torch.int32)[0].item()) if tb.live_ws is not None else int(segments)
    o, d, t = tb.draw_rays_o[:B].clone(), tb.draw_rays_d[:B].clone(), tb.draw_targets[:B].clone()
    api.draw_batch(tb.image_set, B, 0, None, o, d, t)
    stages = tb.time_stages(o, d, t, steps=5)
    diff = {k: [y - x for x, y in zip(ms["plain"], ms[k])] for k in ("ray_gradients", "refine_poses")}
    out = {"rays": B, "frames": f"{a.frames} x {res}x{res} RGB", "reps": a.reps, "steps_per_rep": a.steps,
           "ms_per_step": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
           "minus_plain_ms": {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                              for k, v in diff.items()},
           "eager_stage_ms": {k: round(stages[k], 4) for k in ("encode", "hash_bwd", "ray_grad") if k in stages},
           "segments_last_step": int(segments), "live_segments_last_step": live,
           "live_share": round(live / max(1, int(segments)), 4),
           "pose_updates_min": int(tc.pose_updates.min().item()), "pose_delta_max": float(tc.pose_delta.abs().max().item()),
           "truncated_steps": [ta.truncated_steps, tb.truncated_steps, tc.truncated_steps]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
