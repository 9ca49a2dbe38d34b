#!/usr/bin/env python3
"""Train the hash-grid (or frequency) model against an analytic teacher field and report
PSNR on a held-out pose -- exercises the whole training path of rtx_nerf_amd.train.Trainer.
  python tools/train_demo.py [--steps 300] [--encoding hash|freq] [--grid 32] [--res 64]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rtx_nerf_amd import scenes
from rtx_nerf_amd.train import Trainer, camera_rays


teacher_field = scenes.teacher_field   # kept under this name for the tests that import it from here


def run(steps=300, encoding="hash", grid=32, res=64, batch=4096, n_poses=12, seed=0, verbose=True, neurons=64, layers=2,
        hash_levels=8, hash_log2=15, hash_base=8, background=None, rgba=False, loss="l2", loss_param=None, opacity_weight=0.0,
        probe=None, distortion_weight=0.0, loss_scale=128.0):
    """Returns (PSNR before, PSNR after, losses) on the held-out pose.  background=None, rgba=False: the teacher over black,
    trained over black.  background=(r, g, b): the training targets are the teacher composited over that colour, or with
    rgba=True its straight RGBA (colour / opacity, opacity); "random" (needs rgba): RGBA targets over a fresh background per
    ray and step.  With a background both PSNRs are dicts {"white": dB, "black": dB}: the model against the teacher, both
    composited over white / over black.  loss / loss_param / opacity_weight: the Trainer's; distortion_weight /
    loss_scale likewise.  probe: called as probe(trainer, rays_o, rays_d, targets, when) with the whole training
    set, when = "before" and "after" the steps."""
    if background == "random" and not rgba:
        raise ValueError("train_demo.run: background='random' trains on RGBA targets (rgba=True)")
    torch.cuda.set_device(0)
    dense = scenes.sphere_density(grid, 0.72)
    occ = torch.from_numpy(scenes.pack_occupancy(dense).view(np.int32).copy()).cuda()
    hashgrid = dict(n_levels=hash_levels, n_features=2, log2_hashmap_size=hash_log2, base_resolution=hash_base,
                    per_level_scale=1.5)
    tr = Trainer(grid, occ, encoding=encoding, n_neurons=neurons, n_hidden_layers=layers, hashgrid=hashgrid,
                 batch_rays=max(batch, res * res), max_segments=max(batch, res * res) * 40, lr=1e-2 if encoding == "hash" else 2e-3,
                 loss_scale=loss_scale, density_scale=150.0, mode="nerf", seed=seed, background=background,
                 target_channels=4 if rgba else None, loss=loss, loss_param=loss_param, opacity_weight=opacity_weight,
                 distortion_weight=distortion_weight)

    def teacher(o, d):
        """the training target of these rays"""
        black = tr.render_rays(o, d, radiance_fn=teacher_field).clone()
        if background is None:
            return black
        if not rgba:
            return tr.render_rays(o, d, radiance_fn=teacher_field, background=background).clone()
        # straight RGBA from the renders over black (sum w c) and over white (+ 1 - A)
        alpha = (1.0 - (tr.render_rays(o, d, radiance_fn=teacher_field, background=(1.0, 1.0, 1.0)) - black).mean(1, keepdim=True)).clamp(0, 1)
        rgb = torch.where(alpha > 1e-6, black / alpha.clamp_min(1e-6), torch.zeros_like(black))
        return torch.cat([rgb, alpha], 1).contiguous()

    focal = scenes.lego_focal_length(True)
    rays_o, rays_d, targets = [], [], []
    for i in range(n_poses):
        la = scenes.pose_spherical(360.0 * i / n_poses, -20.0 - 25.0 * (i % 3), origin_scale=10.0)
        o, d = camera_rays(la, focal, res, res)
        rays_o.append(o); rays_d.append(d); targets.append(teacher(o, d))
    rays_o, rays_d, targets = torch.cat(rays_o), torch.cat(rays_d), torch.cat(targets)
    la_test = scenes.pose_spherical(77.0, -33.0, origin_scale=10.0)
    o_t, d_t = camera_rays(la_test, focal, res, res)
    evals = {None: None} if background is None else {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}
    gt_t = {k: tr.render_rays(o_t, d_t, radiance_fn=teacher_field, background=b).clone() for k, b in evals.items()}

    def psnr():
        out = {}
        for k, b in evals.items():
            pred = tr.render_rays(o_t, d_t, background=b)
            mse = float(((pred - gt_t[k]) ** 2).mean())
            out[k] = 10 * np.log10(1.0 / max(mse, 1e-12))
        return out[None] if background is None else out

    g = torch.Generator(device="cuda").manual_seed(seed)
    p0 = psnr()
    if probe is not None:
        probe(tr, rays_o, rays_d, targets, "before")
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(steps):
        idx = torch.randint(0, rays_o.shape[0], (batch,), device="cuda", generator=g)
        loss = tr.step(rays_o[idx].contiguous(), rays_d[idx].contiguous(), targets[idx].contiguous())
        if it % 50 == 0 or it == steps - 1:
            losses.append(float(loss.item()))
            if verbose:
                print(f"step {it:4d} loss {losses[-1]:.6f}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    p1 = psnr()
    if probe is not None:
        probe(tr, rays_o, rays_d, targets, "after")
    if verbose:
        fmt = (lambda p: f"{p:.2f}") if background is None else (lambda p: " / ".join(f"{k} {v:.2f}" for k, v in p.items()))
        print(f"encoding={encoding} steps={steps} batch={batch}{'' if background is None else f' background={background} rgba={rgba}'}: "
              f"PSNR {fmt(p0)} -> {fmt(p1)} dB; "
              f"{steps * batch / dt / 1e6:.3f} Mrays/s trained ({1e3 * dt / steps:.2f} ms/step)")
    return p0, p1, losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--encoding", default="hash")
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--neurons", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--hash-levels", type=int, default=8)
    ap.add_argument("--hash-log2", type=int, default=15)
    ap.add_argument("--hash-base", type=int, default=8)
    a = ap.parse_args()
    run(a.steps, a.encoding, a.grid, a.res, a.batch, neurons=a.neurons, layers=a.layers, hash_levels=a.hash_levels,
        hash_log2=a.hash_log2, hash_base=a.hash_base)
