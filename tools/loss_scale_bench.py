#!/usr/bin/env python3
"""What the dynamic loss scale and gradient-norm clipping cost per training step.  One JSON line per model: ms per
captured step of five trainers on the same rays, targets and weights,
  (a) guard          skip_nonfinite alone at a fixed scale: check_gradients_kernel, optimizer_rate_kernel and the by-value _opt Adam
                     kernels -- DESIGN 5.13's row (c), measured again here;
  (b) dynamic        loss_scale=api.loss_scaler(...): gradient_statistics_kernel in place of the check, loss_scaler_kernel in place
                     of the rate kernel, the compositor and the Adam kernels reading their factor from the device;
  (c) dynamic_clip   (b) with max_grad_norm set (the same launches: the multiplier is another number);
  (a') guard_huber, (b') dynamic_huber    (a) and (b) with loss="huber", so that both run the compositor TEMPLATE -- with the
                     default L2, (a) runs volrender_l2's hard-wired kernel and (b) the template, and (b) - (a) carries that difference,
and three kernels alone over the trainer's gradient buffers (launch + kernel): the check, the statistics, the scaler step.
Models, the checkpoint start, the capture at a learning rate of 0, the alternation of rows and the paired differences are
tools/optimizer_bench.py's.
  python tools/loss_scale_bench.py [--reps 7] [--steps 200] [--pretrain 100] [--models config3,ref8x128]"""
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
NEVER = dict(init_scale=128.0, growth_interval=10 ** 9)      # the scale stays at the fixed rows' 128 for the whole measurement
ROWS = {"guard": dict(skip_nonfinite=True), "dynamic": dict(loss_scale=NEVER), "dynamic_clip": dict(loss_scale=NEVER, max_grad_norm=1e-3),
        "guard_huber": dict(skip_nonfinite=True, loss="huber"), "dynamic_huber": dict(loss_scale=NEVER, loss="huber")}


def trainer(model, occ, **kw):
    kw.setdefault("loss_scale", 128.0)
    if model == "config3":
        return Trainer(128, occ, encoding="hash", n_neurons=64, n_hidden_layers=4,
                       hashgrid=dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5),
                       n_dir_freqs=4, batch_rays=B, max_segments=B * 10, lr=1e-2, density_scale=300.0, mode="nerf", **kw)
    return Trainer(128, occ, encoding="freq", n_neurons=128, n_hidden_layers=8, n_dir_freqs=12, batch_rays=B, max_segments=B * 10, lr=1e-3,
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


def measure(model, occ, a):
    focal = scenes.lego_focal_length(True)
    trs = {k: trainer(model, occ, **kw) for k, kw in ROWS.items()}
    ta = trs["guard"]
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
    # the two new kernels alone, on a scaler and options of their own (the trainers' state is not touched)
    cfg = api.loss_scaler(**NEVER)
    sc_state, sc_ws = api.loss_scaler_state_tensor(cfg), api.loss_scaler_workspace()
    sc = api.loss_scaler(**NEVER, state=sc_state, partials=sc_ws)
    opt = api.optimizer_options(None, 0.0, True, torch.ones(1, device="cuda"), flag)
    k_step, k_rate = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    rows["kernel_statistics"] = lambda: api.gradient_statistics(grads, flag, sc)
    rows["kernel_scaler_step"] = lambda: api.loss_scaler_step(opt, sc, grads, k_step, k_rate[0:1], lr=0.0, table_effective_lr=k_rate[1:2])

    for fn in rows.values():                       # warm-up: every shape the timed windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, fn in rows.items():
            ms[k].append(timed(fn, a.steps))

    def paired(y, base="guard"):
        diff = [q - p for p, q in zip(ms[base][1:], ms[y][1:])]
        return {"median": round(float(np.median(diff)), 4), "min": round(min(diff), 4), "max": round(max(diff), 4)}

    warm = ms["guard"][1:]
    return {"model": model, "rays": B, "reps": a.reps, "steps_per_rep": a.steps, "pretrain_steps": a.pretrain,
            "segments": int(ta.total.item()), "gradient_bytes_checked": int(sum(g.numel() * g.element_size() for g in grads)),
            "skipped_steps": {k: int(tr.skipped_steps.item()) for k, tr in trs.items() if tr.skipped_steps is not None},
            "truncated_steps": [tr.truncated_steps for tr in trs.values()],
            "ms_per_step": {k: {"median": round(float(np.median(v)), 4), "reps": [round(x, 4) for x in v]} for k, v in ms.items()},
            "loss_scale_now": {k: float(tr.loss_scale_now.item()) for k, tr in trs.items() if tr.loss_scale_now is not None},
            "clipped_steps": {k: int(tr.clipped_steps.item()) for k, tr in trs.items() if tr.clipped_steps is not None},
            "grad_norm": {k: float(tr.grad_norm.item()) for k, tr in trs.items() if tr.grad_norm is not None},
            "guard_spread_without_first_rep_ms": {"min": round(min(warm), 4), "max": round(max(warm), 4)},
            "minus_guard_ms": {k: paired(k) for k in ("dynamic", "dynamic_clip")},
            "dynamic_huber_minus_guard_huber_ms": paired("dynamic_huber", "guard_huber"),
            "kernel_statistics_minus_kernel_check_ms": paired("kernel_statistics", "kernel_check")}


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
