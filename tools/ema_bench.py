#!/usr/bin/env python3
"""What the weight EMA costs per training step.  One JSON line per model: ms per captured step of three trainers on
the same rays, targets and weights,
  (a) off      no ema_decay: the kernels and launches of a step as it was;
  (b) ema      ema_decay=0.99: optimizer_rate_kernel + adam_ema_kernel on the MLP + adam_sparse_ema_kernel on the table (the lazy
               form: accumulator and stamps move only for the quads Adam touches);
  (c) options  a one-step warm-up, i.e. active options whose factor is 1: optimizer_rate_kernel + the _opt Adam kernels -- the
               path (b) is a sibling of, so (b) - (c) is the EMA's own share of (b) - (a),
and the read-out alone, rtxn_ema_weights over the full table and over the MLP into fp16 (launch + kernel) -- what sync_ema() pays
per call, and per element what a dense EMA pass over the table would pay per STEP.
Models and protocol are tools/optimizer_bench.py's: "config3" -- 4096 rays, hash grid (16 levels, 2^19 entries, 2 features: the
25 MB table) + 4x64 MLP, 128^3 stand-in occupancy -- and "ref8x128", the reference's 8 x 128 frequency model on the same rays.
All trainers start from one checkpoint (`--pretrain` eager steps of (a)) and are captured with a learning rate of 0, so every
row runs its step on the same weights and samples for the whole measurement (Adam still loads and stores every entry it touches,
and the EMA line runs in full).  Rows run in alternation, `reps` times `steps` back-to-back replays each between HIP events; the
line carries every repetition, the medians, and the paired difference to (a) beside (a)'s own spread without its first (cold)
repetition, which is what a claim about it has to clear.
  python tools/ema_bench.py [--reps 7] [--steps 200] [--pretrain 100] [--models config3,ref8x128] [--decay 0.99]"""
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
from rtx_nerf_amd.train import camera_rays
from optimizer_bench import B, timed, trainer
from train_demo import teacher_field


def measure(model, occ, a):
    focal = scenes.lego_focal_length(True)
    trs = {"off": trainer(model, occ), "ema": trainer(model, occ, ema_decay=a.decay),
           "options": trainer(model, occ, lr_schedule=dict(warmup_steps=1))}
    ta, te = trs["off"], trs["ema"]
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
    hash_ = te.encoding == "hash"
    mlp16 = torch.empty_like(te.params)
    rows["kernel_readout_mlp"] = lambda: api.ema_weights(te.master, te.ema_mlp, None, te._ema_state, a.decay, out_f16=mlp16)
    if hash_:
        table16 = torch.empty_like(te.table)
        rows["kernel_readout_table"] = lambda: api.ema_weights(te.table_master, te.ema_table, te.ema_stamps, te._ema_state, a.decay, out_f16=table16)

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
    touched = int((te.ema_stamps == int(te.ema_updates.item())).sum().item()) if hash_ else 0
    return {"model": model, "rays": B, "reps": a.reps, "steps_per_rep": a.steps, "pretrain_steps": a.pretrain, "decay": a.decay,
            "segments": int(ta.total.item()), "ema_updates": int(te.ema_updates.item()),
            "mlp_params": te.master.numel(), "table_params": te.table_master.numel() if hash_ else 0,
            "table_params_touched_by_the_last_step": touched,
            "dense_table_ema_bytes_per_step_estimate": 8 * (te.table_master.numel() if hash_ else 0),
            "truncated_steps": [tr.truncated_steps for tr in trs.values()],
            "ms_per_step": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
            "off_spread_without_first_rep_ms": {"min": round(min(warm), 4), "max": round(max(warm), 4)},
            "ema_minus_off_ms": paired("off", "ema"), "options_minus_off_ms": paired("off", "options"),
            "ema_minus_options_ms": paired("options", "ema")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--pretrain", type=int, default=100)
    ap.add_argument("--models", default="config3,ref8x128")
    ap.add_argument("--decay", type=float, default=0.99)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(128, seed=0)).view(np.int32).copy()).cuda()
    for model in a.models.split(","):
        print(json.dumps(measure(model, occ, a)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
