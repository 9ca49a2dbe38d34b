#!/usr/bin/env python3
"""Which distortion weight and loss scale the sphere teacher takes (the thresholds of
tests/test_gpu_distortion.py::test_training_with_the_regulariser come from here).  tools/train_demo.py's run -- 300 steps, hash
model, seed 0 -- once per (loss_scale, distortion_weight); one line each: held-out PSNR before -> after, the mean L_r over the
held-out pose's 4096 rays before -> after, first -> last loss.
  python tools/distortion_sweep.py [--steps 300] [--loss-scales 128,4096] [--weights 0,0.003,0.01,0.03,0.1,0.5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from rtx_nerf_amd import api, scenes
from rtx_nerf_amd.train import camera_rays


def mean_distortion(tr, o, d):
    """mean L_r of the trainer's current model over the given rays: its own traversal and forward (gradients(): no optimizer
    step), the write pass repeated with t_start / t_end, and the compositor with weight 0 and the L_r output"""
    n = o.shape[0]
    tgt = torch.zeros((n, 3), device="cuda")
    tr.gradients(o, d, tgt)
    ts, te = torch.zeros(tr.max_segments, device="cuda"), torch.zeros(tr.max_segments, device="cuda")
    api.trace_grid(None, grid_res=tr.R, rays_o=o, rays_d=d, width=n, height=1, ray_begin=0, ray_count=n, occupancy=tr.occ,
                   occupancy_coarse=tr.coarse, occupancy_bricks=tr.bricks, occupancy_super=tr.super_mip, mode=api.TRACE_DDA,
                   viewing_direction=tr.view_dirs, num_hits=tr.num_hits, sub_rays=api.auto_sub_rays(n), sub_hits=tr.sub_hits,
                   indices=tr.indices, start_points=tr.start, end_points=tr.end, seg_view=tr.seg_view, num_stored=tr.num_stored,
                   segment_capacity=tr.max_segments, t_start=ts, t_end=te)
    L = torch.zeros(n, device="cuda")
    pix, lg, loss = torch.zeros((n, 3), device="cuda"), torch.zeros((n, 3), dtype=torch.float16, device="cuda"), torch.zeros(1, device="cuda")
    api.volrender_reg_train(tr.radiance, tr.t_vals, tr.num_stored, tr.indices, n, 32, tgt, tr.loss_scale, pix, lg, loss, torch.empty_like(tr.dout),
                            None, None, api.train_regularizer(0.0, ts, te, distortion=L))
    torch.cuda.synchronize()
    return float(L.mean().item())


def main():
    import train_demo
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--loss-scales", default="128,4096")
    ap.add_argument("--weights", default="0,0.003,0.01,0.03,0.1,0.5")
    a = ap.parse_args()
    o, d = camera_rays(scenes.pose_spherical(77.0, -33.0, origin_scale=10.0), scenes.lego_focal_length(True), 64, 64)
    for ls in (float(v) for v in a.loss_scales.split(",")):
        for lam in (float(v) for v in a.weights.split(",")):
            L = {}

            def probe(tr, rays_o, rays_d, targets, when):
                L[when] = mean_distortion(tr, o, d)

            p0, p1, losses = train_demo.run(steps=a.steps, encoding="hash", verbose=False, probe=probe, distortion_weight=lam, loss_scale=ls)
            print(f"loss_scale {ls:g} distortion_weight {lam:g}: PSNR {p0:.2f} -> {p1:.2f} dB  mean L_r {L['before']:.4e} -> {L['after']:.4e}  "
                  f"loss {losses[0]:.4e} -> {losses[-1]:.4e}", flush=True)


if __name__ == "__main__":
    main()
