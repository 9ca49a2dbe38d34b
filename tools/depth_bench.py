#!/usr/bin/env python3
"""What depth supervision costs per training step.  One JSON line: ms per step of two captured steps on the
configs[2]-shaped trainer (4096 rays, hash grid + 4x64 MLP, 128^3 stand-in occupancy) drawing their batches on the device from
one resident image set with depth maps, and the compositor kernels alone:
  (a) off            depth_weight = 0: the draw, rtxn_volrender_l2_train's kernel, the step as it was;
  (b) on             depth_weight = --weight: the draw, rtxn_depth_targets behind it, composite_train_multi_kernel<true, 4, false, true>,
                     and the traversal's write pass stores t_start / t_end;
  (c) kernel_l2 / kernel_depth: api.volrender_l2_train against api.volrender_depth_train (the same weight, D_r written) on the
      same radiance, step lengths and targets (launch + kernel).
Both trainers run at the same --loss-scale, start from one checkpoint (`--pretrain` eager steps of trainer (a)) and are captured
with a learning rate of 0, so both rows run their step on the same weights for the whole measurement.  Rows run in alternation,
`reps` times `steps` back-to-back replays each between HIP events; the line carries every repetition, the medians, and the paired
differences to (a) beside (a)'s own spread without its first (cold) repetition, which is what a claim about them has to clear.
That (a) is the step of the build before the term existed is shown by the kernels' machine code (profiles/r25), not by a timing.
  python tools/depth_bench.py [--reps 7] [--steps 200] [--pretrain 100] [--weight 0.1] [--loss-scale 128]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from rtx_nerf_amd import api, scenes
from rtx_nerf_amd.train import Trainer

B, RES, FRAMES = 4096, 64, 4


def trainer(occ, loss_scale, **kw):
    return Trainer(128, occ, encoding="hash", n_neurons=64, n_hidden_layers=4,
                   hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                   n_dir_freqs=4, batch_rays=B, max_segments=B * 10, lr=1e-2, loss_scale=loss_scale, density_scale=300.0, mode="nerf", **kw)


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
    ap.add_argument("--pretrain", type=int, default=100)
    ap.add_argument("--weight", type=float, default=0.1)
    ap.add_argument("--loss-scale", type=float, default=128.0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(128, seed=0)).view(np.int32).copy()).cuda()
    focal = scenes.lego_focal_length(True)
    # a resident set: random colours (the timing does not depend on them) and 16-bit depth maps in millimetres of the poses' unit,
    # 3 .. 5 units from the camera, every eighth pixel without a measurement
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (FRAMES, RES, RES, 3), dtype=np.uint8)
    depth = rng.integers(30000, 50000, (FRAMES, RES, RES)).astype(np.uint16)
    depth.reshape(-1)[::8] = 0
    poses = np.stack([np.asarray(scenes.pose_spherical(90.0 * i + 15.0, -30.0, origin_scale=10.0), np.float32).reshape(16)
                      for i in range(FRAMES)])
    iset = api.ImageSet(torch.from_numpy(frames).cuda(), torch.from_numpy(poses).cuda(), focal, depth=torch.from_numpy(depth).cuda(),
                        depth_unit=1e-3, depth_kind="z")
    trs = {"off": trainer(occ, a.loss_scale).attach_images(iset), "on": trainer(occ, a.loss_scale, depth_weight=a.weight).attach_images(iset)}
    ta = trs["off"]
    for _ in range(a.pretrain):
        ta.step_images()
    with tempfile.TemporaryDirectory() as tmp:
        ta.save_checkpoint(os.path.join(tmp, "start.ckpt"))
        for tr in trs.values():
            tr.load_checkpoint(os.path.join(tmp, "start.ckpt"))
    for tr in trs.values():
        tr.lr = 0.0                                 # the weights stay the checkpoint's in both rows
        tr.capture_step(B, launch_segments=tr.max_segments, draw=True)
    rows = {k: tr.step_captured for k, tr in trs.items()}

    # (c): the two compositor kernels on trainer (b)'s buffers as its last step leaves them
    tb = trs["on"]
    tb.step_captured()
    torch.cuda.synchronize()
    K = api.NUM_SAMPLES_PER_SEGMENT
    t = tb._g_sets[0]["targets"]
    pix, lg = torch.zeros((B, 3), device="cuda"), torch.zeros((B, 3), dtype=torch.float16, device="cuda")
    loss, out, D = torch.zeros(1, device="cuda"), torch.zeros_like(tb.dout), torch.zeros(B, device="cuda")
    dep = api.train_depth(a.weight, "l2", None, tb.depth_targets, tb.t_start, tb.t_end, D)
    comp = (tb.radiance, tb.t_vals, tb.num_stored, tb.indices, B, K, t, a.loss_scale, pix, lg, loss, out)
    rows["kernel_l2"] = lambda: api.volrender_l2_train(*comp)
    rows["kernel_depth"] = lambda: api.volrender_depth_train(*comp, None, None, None, None, dep)

    for fn in rows.values():                       # warm-up: every shape the timed windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, fn in rows.items():
            ms[k].append(timed(fn, a.steps))

    def paired(x, y):
        diff = [q - p for p, q in zip(ms[x][1:], ms[y][1:])]
        return {"median": round(float(np.median(diff)), 4), "min": round(min(diff), 4), "max": round(max(diff), 4)}

    warm = ms["off"][1:]
    res = {"rays": B, "reps": a.reps, "steps_per_rep": a.steps, "pretrain_steps": a.pretrain, "depth_weight": a.weight,
           "loss_scale": a.loss_scale, "segments": int(tb.total.item()),
           "rays_with_target": int((tb.depth_targets > 0).sum().item()),
           "truncated_steps": [tr.truncated_steps for tr in trs.values()],
           "ms_per_step": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
           "off_spread_without_first_rep_ms": {"min": round(min(warm), 4), "max": round(max(warm), 4)},
           "on_minus_off_ms": paired("off", "on"), "kernel_depth_minus_kernel_l2_ms": paired("kernel_l2", "kernel_depth")}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
