#!/usr/bin/env python3
"""Cost of the depth / opacity / background outputs on the bench frame (800x800, 128^3 Lego stand-in, 8x128 MLP, four poses),
all in one process: the plain compositor (rtxn_volrender_fwd_compact) against rtxn_volrender_fwd_aux on the same frame's
slot buffers (HIP events, median of --iters), and the whole pipelined frame (render_async) against render_async_ex with depth,
opacity and a white background (RenderPipeline(aux=True)), in alternating rounds.  Prints one JSON line.
  python tools/aux_bench.py [--iters 50] [--frames 20] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rtx_nerf_amd import api, render, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
torch.cuda.set_device(0)
W, H, R, K = 800, 800, 128, api.NUM_SAMPLES_PER_SEGMENT
occ = torch.from_numpy(scenes.pack_occupancy(scenes.lego_standin_density(R, seed=0)).view(np.int32).copy()).cuda()
net = api.Network(n_neurons=128, n_hidden_layers=8)
net.set_params(torch.from_numpy(scenes.xavier_params_fp16(128, 8, net.encoded_width(), seed=1337)).cuda())
focal = scenes.lego_focal_length(True)
poses = [scenes.pose_spherical(360.0 * i / 4 + 15.0, -30.0, origin_scale=10.0) for i in range(4)]
poses_d = [torch.from_numpy(p.reshape(16)).cuda() for p in poses]
plain = render.RenderPipeline(net, R, W, H, focal, occupancy=occ, max_segments=1024, stable_inputs=True)
aux = render.RenderPipeline(net, R, W, H, focal, occupancy=occ, max_segments=1024, stable_inputs=True, aux=True)
plain.calibrate(poses)
aux.calibrate(poses)
n = W * H
WHITE = (1.0, 1.0, 1.0)


def event_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


# ---- compositor kernels on one frame's slot buffers (pose 0)
aux.set_pose(poses[0])
aux.render_ex(background=WHITE)
torch.cuda.synchronize()
P = int(aux.total.item())
t_start = torch.linspace(3.0, 5.0, P, device="cuda")       # the timing does not depend on the distances' values
t_end = t_start + 0.02
pix, dep, acc = torch.empty((n, 3), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
g = aux._slots[0]
kern = {
    "plain": event_ms(lambda: api.volrender_compact(g.radiance, g.num_hits_c, g.indices, n, K, pix), a.iters),
    "aux_opacity_bg": event_ms(lambda: api.volrender_fwd_aux(g.radiance, None, g.num_hits_c, g.indices, n, K, pix,
                                                             opacity=acc, background=WHITE), a.iters),
    "aux_all": event_ms(lambda: api.volrender_fwd_aux(g.radiance, None, g.num_hits_c, g.indices, n, K, pix, t_start=t_start,
                                                      t_end=t_end, depth=dep, opacity=acc, background=WHITE), a.iters),
}


# ---- whole pipelined frames, plain and aux in alternating rounds
def frames(pipe, ex):
    outs = [(torch.empty((n, 3), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")) for _ in range(2)]
    for i in range(3):
        (pipe.render_async_ex(poses_d[i % 4], background=WHITE, out=outs[i & 1]) if ex else
         pipe.render_async(poses_d[i % 4], out=outs[i & 1][0]))
    pipe.drain_async()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.frames):
        (pipe.render_async_ex(poses_d[i % 4], background=WHITE, out=outs[i & 1]) if ex else
         pipe.render_async(poses_d[i % 4], out=outs[i & 1][0]))
    pipe.drain_async()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / a.frames


fr = {"plain": [], "aux": []}
for _ in range(a.rounds):
    fr["plain"].append(frames(plain, False))
    fr["aux"].append(frames(aux, True))
assert not plain.overflowed() and not aux.overflowed()
rec = {
    "frame": f"{W}x{H}, {R}^3 Lego stand-in, 8x128 MLP, {P} segments (pose 0)",
    "compositor_ms": {k: round(v, 4) for k, v in kern.items()},
    "compositor_ratio_aux_all": round(kern["aux_all"] / kern["plain"], 3),
    "frame_ms": {k: [round(x, 3) for x in v] for k, v in fr.items()},
    "frame_ratio_aux_median": round(float(np.median(fr["aux"])) / float(np.median(fr["plain"])), 4),
}
print(json.dumps(rec))
