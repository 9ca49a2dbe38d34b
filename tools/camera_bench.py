#!/usr/bin/env python3
"""What the camera models cost.  One JSON line, on the configs[2]-shaped trainer (hash grid + 4x64 MLP, 128^3
stand-in occupancy):
  draw_*          api.draw_batch alone at 4096 rays from `frames` uint8 frames of res x res: rtxn_draw_batch (the set's pinhole)
                  and rtxn_draw_batch_cameras with a pinhole, an OPENCV and an OPENCV_FISHEYE set (one camera per image);
  frame_pose      the evaluation pipeline's render() at res x res, the pose read from the image set: rtxn_render_frame;
  frame_rays      rtxn_render_frame_rays over rays generated once (the frame alone over explicit rays);
  frame_camera    render_camera(): rtxn_camera_rays + rtxn_render_frame_rays with the centred pinhole that is the pose frame's camera;
  camera_rays     rtxn_camera_rays alone at res x res, each model.
The rows run in alternation, `reps` times, each over `steps` calls between HIP events; the line carries every repetition, the
medians, and the spread of the paired differences against the pinhole draw resp. the pose frame, which is what a claim about them has
to clear.
  python tools/camera_bench.py [--reps 7] [--steps 200] [--frame-steps 40] [--frames 8] [--res 800]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from rtx_nerf_amd import api, scenes
from rtx_nerf_amd.train import Trainer

B = 4096
OPENCV = dict(k1=-0.3, k2=0.1, k3=-0.01, p1=0.001, p2=-0.001)
FISHEYE = dict(k1=-0.02, k2=0.003, k3=-0.001, k4=0.0001)


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
    ap.add_argument("--frame-steps", type=int, default=40)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--res", type=int, default=800)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res, n = a.res, a.frames
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(128, seed=0)).view(np.int32).copy()).cuda()
    focal = scenes.lego_focal_length(True)
    tr = Trainer(128, occ, encoding="hash", n_neurons=64, n_hidden_layers=4,
                 hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                 n_dir_freqs=4, batch_rays=B, max_segments=B * 10, lr=1e-2, loss_scale=128.0, density_scale=300.0, mode="nerf")
    poses = torch.from_numpy(np.stack([np.asarray(scenes.pose_spherical(360.0 * i / n + 15.0, -30.0, origin_scale=10.0), np.float32)
                                       for i in range(n)])).cuda()
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, res, res, 3), dtype=np.uint8)).cuda()
    f_px = focal * res / 2                                    # the centred pinhole of the set's focal length
    centred = api.camera_params(f_px, f_px, res / 2, res / 2)
    sets = {"pinhole": api.ImageSet(img, poses, focal)}
    cams = {}
    for name, model, extra in (("cameras_pinhole", "pinhole", {}), ("cameras_opencv", "opencv", OPENCV), ("cameras_fisheye", "opencv_fisheye", FISHEYE)):
        rows = [api.camera_params(f_px + i, f_px - i, res / 2 + i, res / 2 - i, **extra) for i in range(n)]
        cams[name] = api.camera_set(model, rows, width=res, height=res)
        sets[name] = api.ImageSet(img, poses, cameras=cams[name])
    o, d, t = (torch.empty((B, 3), device="cuda") for _ in range(3))
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = {f"draw_{k}": ((lambda s=s: api.draw_batch(s, B, 0, step, o, d, t)), a.steps) for k, s in sets.items()}

    held = sets["pinhole"]
    rec = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    tr.evaluate(held, out=rec)                                  # builds and calibrates the pipeline
    pipe = next(iter(tr._eval_pipelines.values()))[0]
    one = api.camera_set("pinhole", centred, width=res, height=res)
    ro, rd = api.camera_rays(one, 0, poses[0], res, res)
    frame = [0]

    def row_pose():
        pipe.render(look_at=poses[frame[0] % n])
        frame[0] += 1

    def row_camera():
        pipe.render_camera(one, 0, poses[frame[0] % n])
        frame[0] += 1

    rows["frame_pose"] = (row_pose, a.frame_steps)
    rows["frame_rays"] = (lambda: pipe.render_rays(ro, rd), a.frame_steps)
    rows["frame_camera"] = (row_camera, a.frame_steps)
    co, cd = torch.empty((res * res, 3), device="cuda"), torch.empty((res * res, 3), device="cuda")
    for name, cs in (("pinhole", one), ("opencv", cams["cameras_opencv"]), ("fisheye", cams["cameras_fisheye"])):
        rows[f"camera_rays_{name}"] = ((lambda cs=cs: api.camera_rays(cs, 0, poses[0], res, res, rays_o=co, rays_d=cd)), a.steps)
    for fn, _ in rows.values():                                 # warm-up: every shape the timed windows use
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, (fn, steps) in rows.items():
            ms[k].append(timed(fn, steps))

    def paired(x, y):
        diff = [q - p for p, q in zip(ms[x], ms[y])]
        return {"median": round(float(np.median(diff)), 4), "min": round(min(diff), 4), "max": round(max(diff), 4)}

    out = {"rays": B, "frames": f"{n} x {res}x{res} RGB8", "reps": a.reps, "steps_per_rep": a.steps, "frames_per_rep": a.frame_steps,
           "segments_last_frame": int(pipe.total.item()), "overflowed": bool(pipe.overflowed()),
           "ms": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
           "minus_draw_pinhole_ms": {k: paired("draw_pinhole", f"draw_{k}") for k in cams},
           "minus_frame_pose_ms": {k: paired("frame_pose", k) for k in ("frame_rays", "frame_camera")}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
