#!/usr/bin/env python3
"""Trainer.refresh_occupancy() (rtxn_occupancy_refresh: one device-side call) against Trainer.update_occupancy() (the Python
loop over the staged training route) at 128^3, same process, same box.

Two models, as bench.py / bench_train.py build them:
  hash   BASELINE.json configs[2]: hash grid L=16 F=2 T=2^19 + Frequency(4) directions + 4x64;
  freq   the reference's own model: Composite-Frequency(3 x 10, 2 x 12) + 8x128.

Each call is timed with HIP events on the current stream (update_occupancy() ends in a host read, so its figure includes the
round trips it forces; refresh_occupancy() makes none), --runs timed calls after --warmup untimed ones, the two alternating;
medians and the spread are reported.  refresh_occupancy() is timed as a plain point sample (decay 0, no jitter, absolute
threshold: what update_occupancy() computes) and in its default form (EMA, jitter, min(threshold, mean)), and once more
replayed from a captured graph.  --update-only times update_occupancy() alone and accepts a library from before this entry
point (RTXN_LIB_PATH): the comparison point on the parent commit.

    python tools/occupancy_refresh_bench.py > profiles/r06/occupancy_refresh.txt
    RTXN_LIB_PATH=/path/to/parent/librtxn.so python tools/occupancy_refresh_bench.py --update-only
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

NEW = ["rtxn_occupancy_refresh_supported", "rtxn_occupancy_refresh_workspace_bytes", "rtxn_occupancy_refresh"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="hash,freq")
    ap.add_argument("--grid-res", type=int, default=128)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--update-only", action="store_true")
    return ap.parse_args()


def build(kind, R):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(R, seed=0)).view(np.int32).copy()).cuda()
    B = 4096
    if kind == "hash":
        hgd = dict(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5)
        return Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=4, hashgrid=hgd, n_dir_freqs=4, batch_rays=B,
                       max_segments=B * 16, density_scale=300.0, mode="nerf")
    return Trainer(R, occ, encoding="freq", n_neurons=128, n_hidden_layers=8, n_dir_freqs=12, batch_rays=B, max_segments=B * 16,
                   density_scale=300.0, mode="nerf")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def line(name, ms):
    ms = sorted(ms)
    print(f"{name:<44} median {statistics.median(ms):8.3f} ms   min {ms[0]:8.3f}   max {ms[-1]:8.3f}   ({len(ms)} calls)")


def main():
    args = parse()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    has_new = all(hasattr(handle, n) for n in NEW)
    if not has_new:
        if not args.update_only:
            sys.exit("this librtxn.so has no rtxn_occupancy_refresh: --update-only")
        for n in NEW:
            _lib.SYMBOLS.pop(n)
    assert torch.cuda.is_available(), "occupancy_refresh_bench.py needs a GPU"
    R = args.grid_res
    print(f"# librtxn: {os.path.basename(_lib.LIB_PATH)} (rtxn_occupancy_refresh: {'yes' if has_new else 'no'}); {torch.cuda.get_device_name(0)}")
    print(f"# {R}^3 = {R ** 3} cells, threshold {args.threshold}; HIP events around each call, {args.warmup} warm-up + {args.runs} timed "
          f"calls per variant, variants alternating")
    for kind in args.models.split(","):
        tr = build(kind, R)
        print(f"\n## {kind}")
        variants = [("update_occupancy()", lambda: tr.update_occupancy(args.threshold))]
        if not args.update_only:
            point = dict(threshold=args.threshold, decay=0.0, jitter=False, threshold_mode="absolute")
            variants.append(("refresh_occupancy(point sample)", lambda: tr.refresh_occupancy(**point)))
            variants.append(("refresh_occupancy() [EMA, jitter, min_mean]", lambda: tr.refresh_occupancy(threshold=args.threshold)))
            variants.append(("refresh_occupancy(runs_per_pass=8192)", lambda: tr.refresh_occupancy(threshold=args.threshold, runs_per_pass=8192)))
        times = {name: [] for name, _ in variants}
        for it in range(args.warmup + args.runs):
            for name, fn in variants:
                ms = timed(fn)
                if it >= args.warmup:
                    times[name].append(ms)
        for name, _ in variants:
            line(name, times[name])
        if not args.update_only:
            frac_u = tr.update_occupancy(args.threshold)
            tr.occ_density.zero_()
            tr.refresh_occupancy(**point)
            frac_r, mean = tr.occupancy_stats()
            print(f"occupied fraction: update_occupancy {frac_u:.6f}, refresh_occupancy(point sample) {frac_r:.6f}; mean thickness {mean:.4g}")
            # the same call replayed from a graph: what a captured training loop pays
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                tr.refresh_occupancy(threshold=args.threshold)
            ms = []
            for it in range(args.warmup + args.runs):
                t = timed(graph.replay)
                if it >= args.warmup:
                    ms.append(t)
            line("refresh_occupancy() replayed from a graph", ms)
        del tr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
