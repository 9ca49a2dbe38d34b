#!/usr/bin/env python3
"""A/B of early ray termination (RenderPipeline(min_transmittance=...)) against the plain frame, same process, same box.

Two workloads, built as bench.py builds them:
  freq   BASELINE.json configs[1]: 800x800 frame, 128^3 Lego stand-in occupancy, 8x128 frequency model, Xavier weights
         (seed 1337), RTXN_VR_COMPAT;
  hash   the hash-grid render of bench.py's extra_render_hash: the configs[2] model (hash grid L=16 F=2 T=2^19 + Frequency(4)
         directions + 4x64) trained for --train-steps steps on the analytic teacher, RTXN_VR_NERF, density scale 300.

For each workload and each setting (eps in --eps at every schedule in --schedules) the plain and the terminated frame are timed
ALTERNATELY, --runs runs of --frames serial frames each (rtxn_render_frame on one stream, HIP events around the run), and the
medians are reported with the shaded share of segments, the per-round segment counts (from shaded_per_ray and the schedule)
and the PSNR of the terminated frame against the plain one.  Only plain-against-terminated comparisons are meaningful; the
plain frame of ANOTHER build of the library is measured by --plain-only with RTXN_LIB_PATH pointing at it (a build from before
the termination entry points is accepted: their ctypes rows are dropped when the library lacks them).

    python tools/termination_bench.py > profiles/r06/termination_ab.txt
    RTXN_LIB_PATH=/path/to/parent/librtxn.so python tools/termination_bench.py --plain-only
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rtx_nerf_amd import _lib  # noqa: E402

NEW = ["rtxn_render_termination_workspace_bytes", "rtxn_render_set_termination", "rtxn_render_termination_status",
       "rtxn_render_termination_buffers"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="freq,hash")
    ap.add_argument("--eps", default="1e-2,1e-3,1e-4")
    ap.add_argument("--schedules", default="4x5,2x6", help="first_round_segments x rounds, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--plain-only", action="store_true")
    return ap.parse_args()


def build_freq(size):
    from rtx_nerf_amd import api, render, scenes
    R = 128
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(R, seed=0)).view(np.int32).copy()).cuda()
    net = api.Network(n_neurons=128, n_hidden_layers=8)
    net.set_params(torch.from_numpy(scenes.xavier_params_fp16(128, 8, net.encoded_width(), seed=1337)).cuda())
    pipe = render.RenderPipeline(net, R, size, size, scenes.lego_focal_length(True), occupancy=occ, max_segments=1024, n_slots=1)
    pipe._keep = (net, occ)
    return pipe


def build_hash(size, train_steps):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer, camera_rays
    R, B = 128, 4096
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(R, seed=0)).view(np.int32).copy()).cuda()
    hgd = dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5)
    tr = Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=4, hashgrid=hgd, n_dir_freqs=4,
                 batch_rays=128 * 128, max_segments=128 * 128 * 32, lr=1e-2, loss_scale=128.0, density_scale=300.0, mode="nerf")
    focal = scenes.lego_focal_length(True)
    ro, rd, tg = [], [], []
    for i in range(8):
        o, d = camera_rays(scenes.pose_spherical(45.0 * i + 15.0, -30.0, origin_scale=10.0), focal, 128, 128)
        ro.append(o); rd.append(d); tg.append(tr.render_rays(o, d, radiance_fn=scenes.teacher_field).clone())
    ro, rd, tg = torch.cat(ro), torch.cat(rd), torch.cat(tg)
    g = torch.Generator(device="cuda").manual_seed(42)
    for _ in range(train_steps):
        idx = torch.randint(0, ro.shape[0], (B,), device="cuda", generator=g)
        tr.step(ro[idx].contiguous(), rd[idx].contiguous(), tg[idx].contiguous())
    torch.cuda.synchronize()
    pipe = tr.render_pipeline(size, size, focal, max_segments=1024, n_slots=1)
    pipe._keep = (tr, occ)
    return pipe


def time_frames(pipe, frames):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(frames):
        pipe.render()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / frames


def per_round(shaded, s0, n_rounds):
    """Segments of each round, from the per-ray shaded counts and the schedule."""
    out, lo = [], 0
    for k in range(n_rounds):
        q = s0 * 2 ** k if k < n_rounds - 1 else 1 << 30
        out.append(int(np.clip(shaded - lo, 0, q).sum()))
        lo += q
    return out


def main():
    args = parse()
    lib_handle = ctypes.CDLL(_lib.LIB_PATH)
    has_term = all(hasattr(lib_handle, n) for n in NEW)
    if not has_term:
        if not args.plain_only:
            sys.exit("this librtxn.so has no termination entry points: --plain-only")
        for n in NEW:
            _lib.SYMBOLS.pop(n)
    assert torch.cuda.is_available(), "termination_bench.py needs a GPU"
    from rtx_nerf_amd import scenes
    pose = scenes.pose_spherical(15.0, -30.0, origin_scale=10.0)        # bench.py's first pose
    print(f"# librtxn: {_lib.LIB_PATH} (termination entry points: {'yes' if has_term else 'no'}); {torch.cuda.get_device_name(0)}")
    print(f"# {args.size}x{args.size}, serial rtxn_render_frame, {args.runs} runs x {args.frames} frames, medians; plain and terminated alternate")
    for wl in args.workloads.split(","):
        pipe = build_freq(args.size) if wl == "freq" else build_hash(args.size, args.train_steps)
        total = pipe.calibrate([pose])
        pipe.set_pose(pose)
        for _ in range(3):
            pipe.render()
        plain = pipe.render().clone()
        torch.cuda.synchronize()
        nh = pipe.num_hits_c.cpu().numpy()
        print(f"\n## {wl}: {total} segments, {int((nh > 0).sum())} of {nh.size} rays hit, {nh[nh > 0].mean():.1f} segments per hitting ray")
        if args.plain_only:
            ms = [time_frames(pipe, args.frames) for _ in range(args.runs)]
            print(f"plain frame: {statistics.median(ms):.3f} ms (runs: {' '.join(f'{m:.3f}' for m in ms)})")
            continue
        print("eps      s0xN  plain ms  term ms  term/plain  shaded share  PSNR dB  max |dpix|  segments per round")
        for sch in args.schedules.split(","):
            s0, N = (int(v) for v in sch.split("x"))
            for eps in (float(e) for e in args.eps.split(",")):
                pipe.set_termination(eps, s0, N)
                for _ in range(2):
                    pipe.render()
                term = pipe.render().clone()
                torch.cuda.synchronize()
                shaded = pipe.shaded_per_ray().cpu().numpy()
                st = pipe.termination_stats()
                assert st["last_shaded_segments"] == int(shaded.sum()) and st["last_total_segments"] == total
                t_plain, t_term = [], []
                for _ in range(args.runs):
                    pipe.set_termination(None)
                    pipe.render()
                    t_plain.append(time_frames(pipe, args.frames))
                    pipe.set_termination(eps, s0, N)
                    pipe.render()
                    t_term.append(time_frames(pipe, args.frames))
                pipe.set_termination(None)
                mse = float(((term - plain) ** 2).mean())
                psnr = 10 * np.log10(1.0 / max(mse, 1e-20))
                mp, mt = statistics.median(t_plain), statistics.median(t_term)
                print(f"{eps:<8g} {s0}x{N}   {mp:8.3f} {mt:8.3f}  {mt / mp:10.3f}  {shaded.sum() / total:12.3f}  {psnr:7.1f}  "
                      f"{float((term - plain).abs().max()):10.2e}  {' '.join(str(v) for v in per_round(shaded, s0, N))}")
        del pipe
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
