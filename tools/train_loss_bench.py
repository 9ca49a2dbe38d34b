#!/usr/bin/env python3
"""What a loss other than L2 costs per training step.  One JSON line: ms per step of three captured steps on the
configs[2]-shaped trainer (4096 rays, hash grid + 4x64 MLP, 128^3 stand-in occupancy), all over a constant white background
with the same RGBA targets, and the compositor kernels alone:
  (a) l2             the L2 step: rtxn_volrender_l2_train_ex's volrender_l2_bg_multi_kernel<4>, as before the losses existed;
  (b) huber          loss="huber": composite_train_multi_kernel<false, 4, false>;
  (c) huber_alpha    loss="huber", opacity_weight=0.1: the same kernel with the alpha term and the opacity store;
  (d) kernel_l2_bg / kernel_loss: api.volrender_l2_train_ex against api.volrender_loss_train (huber, lambda = 0.1, opacities
      written) on the same radiance, step lengths and targets (launch + kernel).
The three trainers start from one checkpoint (`--pretrain` eager L2 steps of trainer (a)) and are captured with a learning
rate of 0, so every row runs its step on the same weights and the same samples for the whole measurement.  Rows run in alternation, `reps` times `steps` back-to-back replays each
between HIP events; the line carries every repetition, the medians, and for (b) and (c) the paired differences to (a) beside
(a)'s own spread without its first (cold) repetition, which is what a claim about them has to clear -- and each row's count of
live segments (those with a non-zero radiance gradient, the only ones the backward visits): the loss decides which gradients
round to zero in fp16, so the rows' backward passes do not do the same work even on the same weights.
  python tools/train_loss_bench.py [--reps 7] [--steps 200] [--pretrain 200]"""
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
WHITE = (1.0, 1.0, 1.0)


def trainer(occ, **kw):
    return Trainer(128, occ, encoding="hash", n_neurons=64, n_hidden_layers=4,
                   hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                   n_dir_freqs=4, batch_rays=B, max_segments=B * 10, lr=1e-2, loss_scale=128.0, density_scale=300.0, mode="nerf",
                   background=WHITE, target_channels=4, **kw)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def rgba_targets(tr, o, d):
    """the teacher's straight RGBA from its renders over black and over white"""
    black = tr.render_rays(o, d, radiance_fn=teacher_field).clone()
    alpha = (1.0 - (tr.render_rays(o, d, radiance_fn=teacher_field, background=WHITE) - black).mean(1, keepdim=True)).clamp(0, 1)
    rgb = torch.where(alpha > 1e-6, black / alpha.clamp_min(1e-6), torch.zeros_like(black))
    return torch.cat([rgb, alpha], 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--pretrain", type=int, default=200)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(128, seed=0)).view(np.int32).copy()).cuda()
    focal = scenes.lego_focal_length(True)
    trs = {"l2": trainer(occ), "huber": trainer(occ, loss="huber"), "huber_alpha": trainer(occ, loss="huber", opacity_weight=0.1)}
    ta = trs["l2"]
    g = torch.Generator(device="cuda").manual_seed(0)
    batches = []
    for i in range(4):
        o, d = camera_rays(scenes.pose_spherical(90.0 * i + 15.0, -30.0, origin_scale=10.0), focal, 64, 64)
        batches.append((o, d, rgba_targets(ta, o, d)))
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

    # (d): the two compositor kernels on trainer (a)'s buffers as its last step leaves them
    ta.step_captured()
    torch.cuda.synchronize()
    K = api.NUM_SAMPLES_PER_SEGMENT
    pix, lg = torch.zeros((B, 3), device="cuda"), torch.zeros((B, 3), dtype=torch.float16, device="cuda")
    loss, out, opa = torch.zeros(1, device="cuda"), torch.zeros_like(ta.dout), torch.zeros(B, device="cuda")
    bg = api.train_background(WHITE, target_channels=4)
    spec = api.train_loss("huber", opacity_weight=0.1, opacity=opa)
    comp = (ta.radiance, ta.t_vals, ta.num_stored, ta.indices, B, K, t, 128.0, pix, lg, loss, out)
    rows["kernel_l2_bg"] = lambda: api.volrender_l2_train_ex(*comp, bg)
    rows["kernel_loss"] = lambda: api.volrender_loss_train(*comp, bg, spec)

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

    warm = ms["l2"][1:]
    out = {"rays": B, "reps": a.reps, "steps_per_rep": a.steps, "pretrain_steps": a.pretrain,
           "segments": int(ta.total.item()), "live_segments": {k: int(tr.live_ws[0].item()) for k, tr in trs.items()},
           "truncated_steps": [tr.truncated_steps for tr in trs.values()],
           "ms_per_step": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
           "l2_spread_without_first_rep_ms": {"min": round(min(warm), 4), "max": round(max(warm), 4)},
           "huber_minus_l2_ms": paired("l2", "huber"), "huber_alpha_minus_l2_ms": paired("l2", "huber_alpha"),
           "kernel_loss_minus_kernel_l2_bg_ms": paired("kernel_l2_bg", "kernel_loss")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
