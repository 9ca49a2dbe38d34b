#!/usr/bin/env python3
"""Which depth weight the few-view sphere teacher takes (the margin of
tests/test_gpu_depth.py::test_depth_supervision_lowers_the_held_out_depth_error comes from here).  The sphere teacher of
tools/train_demo.py seen from `--views` training poses only (3: too few for its geometry), a hash model, fixed seeds,
deterministic mode; the depth targets are the teacher's own expected depth D = sum w m along every training ray (a target only
where the teacher is opaque, A > 0.9), handed to Trainer.step(..., depth_targets=).  One line per weight: the held-out pose's mean
|D - z| over its rays with a target, its PSNR, and the last step's loss split into colour and depth share -- where the depth
share passes the colour's is where the term starts to outweigh it.
  python tools/depth_sweep.py [--steps 300] [--views 3] [--weights 0,0.01,0.03,0.1,0.3,1,3] [--loss-scale 128]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from rtx_nerf_amd import api, scenes
from rtx_nerf_amd.train import Trainer, camera_rays, psnr

OPAQUE = 0.9


def expected_depth(tr, o, d, radiance_fn=None):
    """(pixels, D, A) of the given rays under the trainer's model, or under radiance_fn (the teacher): the trainer's own traversal
    and forward (render_rays), the write pass repeated with t_start / t_end, and rtxn_volrender_fwd_aux's depth and opacity"""
    n = o.shape[0]
    pix = tr.render_rays(o, d, radiance_fn=radiance_fn).clone()
    ts, te = torch.zeros(tr.max_segments, device="cuda"), torch.zeros(tr.max_segments, device="cuda")
    api.trace_grid(None, grid_res=tr.R, rays_o=o, rays_d=d, width=n, height=1, ray_begin=0, ray_count=n, occupancy=tr.occ,
                   occupancy_coarse=tr.coarse, occupancy_bricks=tr.bricks, occupancy_super=tr.super_mip, mode=api.TRACE_DDA,
                   viewing_direction=tr.view_dirs, num_hits=tr.num_hits, sub_rays=api.auto_sub_rays(n), sub_hits=tr.sub_hits,
                   indices=tr.indices, start_points=tr.start, end_points=tr.end, seg_view=tr.seg_view, num_stored=tr.num_stored,
                   segment_capacity=tr.max_segments, t_start=ts, t_end=te)
    D, A = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    api.volrender_fwd_aux(tr.radiance, tr.t_vals, tr.num_stored, tr.indices, n, api.NUM_SAMPLES_PER_SEGMENT, torch.zeros((n, 3), device="cuda"),
                          mode=api.VR_NERF, sample_type=api.SAMPLING_MIDPOINT_WORLD, t_start=ts, t_end=te, depth=D, opacity=A)
    torch.cuda.synchronize()
    return pix, D, A


def targets_of(D, A):
    """the teacher's depth where it is opaque, 0 (no target) elsewhere"""
    return torch.where(A > OPAQUE, D, torch.zeros_like(D)).contiguous()


def run(depth_weight, steps=300, views=3, seed=0, loss_scale=128.0, res=48, batch=2048, grid=32, depth_loss="l2"):
    """Returns dict(depth_err, psnr, loss, depth_share): held-out mean |D - z| over rays with a target, held-out PSNR, the last
    step's loss scalar and the depth term's share of it."""
    torch.cuda.set_device(0)
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(grid, 0.72)).view(np.int32).copy()).cuda()
    B = max(batch, res * res)
    tr = Trainer(grid, occ, encoding="hash", n_neurons=64, n_hidden_layers=2,
                 hashgrid=dict(n_levels=8, n_features=2, log2_hashmap_size=15, base_resolution=8, per_level_scale=1.5),
                 batch_rays=B, max_segments=B * 40, lr=1e-2, loss_scale=loss_scale, density_scale=150.0, mode="nerf", seed=seed,
                 deterministic=True, depth_weight=depth_weight, depth_loss=depth_loss)
    focal = scenes.lego_focal_length(True)
    ro, rd, tg, tz = [], [], [], []
    for i in range(views):
        o, d = camera_rays(scenes.pose_spherical(360.0 * i / views + 10.0, -20.0 - 15.0 * (i % 2), origin_scale=10.0), focal, res, res)
        pix, D, A = expected_depth(tr, o, d, scenes.teacher_field)
        ro.append(o); rd.append(d); tg.append(pix); tz.append(targets_of(D, A))
    ro, rd, tg, tz = torch.cat(ro), torch.cat(rd), torch.cat(tg), torch.cat(tz)
    o_t, d_t = camera_rays(scenes.pose_spherical(77.0, -33.0, origin_scale=10.0), focal, res, res)
    pix_t, D_t, A_t = expected_depth(tr, o_t, d_t, scenes.teacher_field)
    z_t = targets_of(D_t, A_t)
    g = torch.Generator(device="cuda").manual_seed(seed)
    loss = None
    for _ in range(steps):
        idx = torch.randint(0, ro.shape[0], (batch,), device="cuda", generator=g)
        loss = tr.step(ro[idx].contiguous(), rd[idx].contiguous(), tg[idx].contiguous(),
                       tz[idx].contiguous() if depth_weight > 0.0 else None)
    last = float(loss.item())
    share = float(depth_weight * tr.depth_loss[:batch].sum().item() / batch) if depth_weight > 0.0 else 0.0
    pix, D, _ = expected_depth(tr, o_t, d_t)
    has = z_t > 0
    return dict(depth_err=float((D - z_t).abs()[has].mean().item()), psnr=psnr(pix, pix_t), loss=last, depth_share=share,
                rays_with_target=int(has.sum().item()), train_rays_with_target=int((tz > 0).sum().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--weights", default="0,0.01,0.03,0.1,0.3,1,3")
    ap.add_argument("--loss-scale", type=float, default=128.0)
    ap.add_argument("--depth-loss", default="l2")
    a = ap.parse_args()
    for lam in (float(v) for v in a.weights.split(",")):
        r = run(lam, a.steps, a.views, loss_scale=a.loss_scale, depth_loss=a.depth_loss)
        print(f"views {a.views} steps {a.steps} loss_scale {a.loss_scale:g} depth_loss {a.depth_loss} depth_weight {lam:g}: held-out mean |D - z| "
              f"{r['depth_err']:.4e} over {r['rays_with_target']} rays  PSNR {r['psnr']:.2f} dB  last loss {r['loss']:.4e} "
              f"(colour {r['loss'] - r['depth_share']:.4e}, depth {r['depth_share']:.4e})", flush=True)


if __name__ == "__main__":
    main()
