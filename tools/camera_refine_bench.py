#!/usr/bin/env python3
"""What the intrinsics refinement costs.  One JSON line: ms per step of five rows on the configs[2]-shaped trainer
(4096 rays, hash grid + 4x64 MLP, 128^3 stand-in occupancy, 8 frames of 128 x 128 drawn on the device through an OPENCV camera set):
  (a) refine_poses      capture_step(draw=True): step_captured() with attach_images(refine_poses=True) -- the graph as it was;
  (b) cameras_shared    the same plus refine_cameras=True over ONE camera shared by the frames: the fold is a single block;
  (c) cameras_per_image the same over one camera per frame;
  (d) gradients_alone   api.camera_gradients by itself over trainer (c)'s last batch (the per-ray terms and the per-camera fold);
  (e) step_alone        api.camera_step by itself on trainer (c)'s state.
Separate trainers from the same seed over the same frames; the rows run in alternation, `reps` times `steps` back-to-back steps
each between HIP events; the line carries every repetition, the medians and the spread of the paired differences against (a).
  python tools/camera_refine_bench.py [--reps 7] [--steps 200] [--frames 8] [--res 128]"""
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
from rtx_nerf_amd.train import camera_rays
from ray_gradient_bench import B, timed, trainer
from train_demo import teacher_field

LENS = dict(k1=-0.05, k2=0.01, p1=0.001, p2=-0.001)


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
    ta, tb, tc = (trainer(occ, ray_gradients=True) for _ in range(3))
    poses, frames = [], []
    for i in range(a.frames):
        pose = scenes.pose_spherical(360.0 * i / a.frames + 15.0, -30.0, origin_scale=10.0)
        o, d = camera_rays(pose, focal, res, res)
        frames.append(ta.render_rays(o, d, radiance_fn=teacher_field).reshape(res, res, 3).clamp(0, 1).cpu().numpy())
        poses.append(np.asarray(pose, np.float32))
    ds = loader.ImageDataset(np.stack(frames), np.stack(poses), 0.0, res, res, 3, scenes.LEGO_CAMERA_ANGLE_X)
    row = api.camera_params(focal * res / 2, focal * res / 2, res / 2, res / 2, **LENS)
    cap = ta.max_segments
    for tr, n_cameras, refine in ((ta, 1, None), (tb, 1, True), (tc, a.frames, True)):      # a set each: the refinement rewrites it in place
        cams = api.camera_set("opencv", [row] * n_cameras, res, res)
        tr.attach_images(api.ImageSet.from_dataset(ds, storage="u8", cameras=cams)[0], refine_poses=True, refine_cameras=refine)
        tr.capture_step(B, launch_segments=cap, draw=True)

    rows = {"refine_poses": ta.step_captured, "cameras_shared": tb.step_captured, "cameras_per_image": tc.step_captured}
    for fn in rows.values():                       # warm-up: every shape the timed windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    # the two kernels alone, on a copy of trainer (c)'s state: thousands of steps on one gradient would walk its rows to the clamps
    own = {k: v.clone() for k, v in tc._cams._tensors.items() if v is not None and k not in ("drawn", "poses", "skip")}
    alone = api.camera_refinement(tc._cams.model, tc._cams.n_cameras, res, **own)
    rows["gradients_alone"] = lambda: api.camera_gradients(tc.drawn, tc.rays_d_grad, B, tc.image_set.poses, alone)
    rows["step_alone"] = lambda: api.camera_step(alone)
    for k in ("gradients_alone", "step_alone"):
        for _ in range(20):
            rows[k]()
    ms = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, fn in rows.items():
            ms[k].append(timed(fn, a.steps))
    diff = {k: [y - x for x, y in zip(ms["refine_poses"], ms[k])] for k in ("cameras_shared", "cameras_per_image")}
    tb.check_cameras()
    tc.check_cameras()
    out = {"rays": B, "frames": f"{a.frames} x {res}x{res} RGB, opencv", "reps": a.reps, "steps_per_rep": a.steps,
           "ms_per_step": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
           "minus_refine_poses_ms": {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                     for k, v in diff.items()},
           "camera_updates_min": [int(t.camera_updates.min().item()) for t in (tb, tc)],
           "camera_delta_max": [float(t.camera_delta.abs().max().item()) for t in (tb, tc)],
           "truncated_steps": [ta.truncated_steps, tb.truncated_steps, tc.truncated_steps]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
