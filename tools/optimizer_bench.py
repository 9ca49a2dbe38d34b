#!/usr/bin/env python3
"""What the optimizer options cost per training step.  One JSON line per model: ms per captured step of four
trainers on the same rays, targets and weights,
  (a) off       no options: the kernels and launches of a step as it was (adam_kernel / adam_sparse_kernel, the rate from the
                table lookup);
  (b) schedule  lr_schedule="nerf" + weight_decay: optimizer_rate_kernel + the _opt Adam kernels;
  (c) guard     skip_nonfinite alone: check_gradients_kernel over every gradient buffer + (b)'s kernels;
  (d) all       (b) and (c),
and the check kernel alone over the trainer's gradient buffers (launch + kernel).
Models: "config3" -- 4096 rays, hash grid (16 levels, 2^19 entries, 2 features: the 25 MB table) + 4x64 MLP, 128^3 stand-in
occupancy -- and "ref8x128", the reference's 8 x 128 frequency model on the same rays.  All trainers start from one checkpoint
(`--pretrain` eager steps of (a)) and are captured with a learning rate of 0, so every row runs its step on the same weights and
samples for the whole measurement (with lr 0 the decay product is 0 and the multiply-subtract per element is not executed: one
VALU pair in an HBM-bound kernel).  Rows run in alternation, `reps` times `steps` back-to-back replays each between HIP events; the
line carries every repetition, the medians, and the paired differences to (a) beside (a)'s own spread without its first (cold)
repetition, which is what a claim about them has to clear.
  python tools/optimizer_bench.py [--reps 7] [--steps 200] [--pretrain 100] [--models config3,ref8x128]"""
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
from rtx_nerf_amd.train import Trainer, camera_rays
from train_demo import teacher_field

B = 4096
ROWS = {"off": {}, "schedule": dict(lr_schedule="nerf", weight_decay=0.01), "guard": dict(skip_nonfinite=True),
        "all": dict(lr_schedule="nerf", weight_decay=0.01, skip_nonfinite=True)}


def trainer(model, occ, **kw):
    if model == "config3":
        return Trainer(128, occ, encoding="hash", n_neurons=64, n_hidden_layers=4,
                       hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                       n_dir_freqs=4, batch_rays=B, max_segments=B * 10, lr=1e-2, loss_scale=128.0, density_scale=300.0, mode="nerf", **kw)
    return Trainer(128, occ, encoding="freq", n_neurons=128, n_hidden_layers=8, n_dir_freqs=12, batch_rays=B, max_segments=B * 10, lr=1e-3,
                   loss_scale=128.0, density_scale=300.0, mode="nerf", **kw)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def measure(model, occ, a):
    focal = scenes.lego_focal_length(True)
    trs = {k: trainer(model, occ, **kw) for k, kw in ROWS.items()}
    ta = trs["off"]
    batches = []
    for i in range(4):
        o, d = camera_rays(scenes.pose_spherical(90.0 * i + 15.0, -30.0, origin_scale=10.0), focal, 64, 64)
        batches.append((o, d, ta.render_rays(o, d, radiance_fn=teacher_field).clone()))
    for k in range(a.pretrain):
        ta.step(*batches[k % 4])
    with tempfile.TemporaryDirectory() as tmp:
        ta.save_checkpoint(os.path.join(tmp, "start.ckpt"))
        for tr in trs.values():
            tr.load_checkpoint(os.path.join(tmp, "start.ckpt"))
    o, d, t = batches[0]
    for tr in trs.values():
        tr.lr = 0.0                                 # the weights stay the checkpoint's in every row
        tr.capture_step(B, launch_segments=tr.max_segments)
        tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
    rows = {k: tr.step_captured for k, tr in trs.items()}
    tg = trs["guard"]
    grads = [tg.dparams] + ([tg.dtable[:tg.hashed_lo], tg.dtable_h] if (tg.encoding == "hash" and tg.hash_fp16) else
                            [tg.dtable] if tg.encoding == "hash" else [])
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    rows["kernel_check"] = lambda: api.check_gradients(grads, flag)

    for fn in rows.values():                       # warm-up: every shape the timed windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, fn in rows.items():
            ms[k].append(timed(fn, a.steps))

    def paired(y):
        diff = [q - p for p, q in zip(ms["off"][1:], ms[y][1:])]
        return {"median": round(float(np.median(diff)), 4), "min": round(min(diff), 4), "max": round(max(diff), 4)}

    warm = ms["off"][1:]
    return {"model": model, "rays": B, "reps": a.reps, "steps_per_rep": a.steps, "pretrain_steps": a.pretrain,
            "segments": int(ta.total.item()), "gradient_bytes_checked": int(sum(g.numel() * g.element_size() for g in grads)),
            "skipped_steps": {k: int(tr.skipped_steps.item()) for k, tr in trs.items() if tr.skipped_steps is not None},
            "truncated_steps": [tr.truncated_steps for tr in trs.values()],
            "ms_per_step": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
            "off_spread_without_first_rep_ms": {"min": round(min(warm), 4), "max": round(max(warm), 4)},
            "minus_off_ms": {k: paired(k) for k in ("schedule", "guard", "all")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--pretrain", type=int, default=100)
    ap.add_argument("--models", default="config3,ref8x128")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(128, seed=0)).view(np.int32).copy()).cuda()
    for model in a.models.split(","):
        print(json.dumps(measure(model, occ, a)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
