#!/usr/bin/env python3
"""What mesh extraction costs on the device: api.density_lattice and api.isosurface, timed with HIP events.

Model rows: density_lattice at 128^3 and 256^3 nodes on
  hash   BASELINE.json configs[2]: hash grid L=16 F=2 T=2^19 + Frequency(4) directions + 4x64;
  freq   the reference's own model: Composite-Frequency(3 x 10, 2 x 12) + 8x128,
with Xavier weights.  Ideal time: the sample count over the fused inference rates README quotes for whole frames (8x128: 37.7
Mrays/s, hash: 59.5 Mrays/s, both on the 800x800 frame of 100 M samples = 156.25 samples per ray).

Isosurface rows: an analytic sphere (distance field, radius 0.8 of the half width) at 256^3 nodes -- 67 MB, INSIDE the 256 MiB
Infinity Cache -- and at 640^3 nodes -- 1.05 GB, real HBM.  Two calls are timed: counts only (iso_count + iso_scan) and the full
call with exact capacities (iso_count + the two scans + iso_emit), with and without normals; emit = full - counts.  Bytes are
computed from the shapes and are what MUST move: the count pass reads 4 B per node (its 4 B word is written only for the nodes of
64-node chunks the surface crosses, and the row totals are 8 B per row: both left out), the emit pass re-reads 4 B per node and
writes 12 (24 with normals) B per vertex and 12 B per triangle (the words it gathers are again the crossed chunks' only).  GB/s
are set against the 6.29 TB/s measured copy rate of an MI355X.

Protocol: one warm-up per row, then --runs (7) repetitions with the rows ALTERNATING; every repetition is printed, medians
reported.  No thresholds.

    python tools/mesh_bench.py > profiles/r21/mesh_bench.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rtx_nerf_amd import api, scenes  # noqa: E402

COPY_RATE = 6.29e12                     # B/s, measured device copy
RATES = {"freq": 37.7e6 * 156.25, "hash": 59.5e6 * 156.25}      # samples/s of the fused inference frames README quotes


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_rows(rows, runs):
    """rows: [(name, fn)]; one warm-up each, then `runs` alternating repetitions -> {name: [ms]}"""
    for _, fn in rows:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in rows}
    for _ in range(runs):
        for name, fn in rows:
            times[name].append(timed(fn))
    return times


def show(name, ms, extra=""):
    print(f"{name:<46} median {statistics.median(ms):9.3f} ms   [{' '.join(f'{t:.3f}' for t in ms)}]{extra}")


def model(kind):
    if kind == "hash":
        hg = api.HashGrid(16, 2, 19, 16, 1.5, n_dir_freqs=4)
        E = hg.encoded_width()
        net = api.Network(n_neurons=64, n_hidden_layers=4, n_encoded_features=E)
        net.set_params(torch.from_numpy(scenes.xavier_params_fp16(64, 4, E, seed=1)).cuda())
        table = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, hg.n_params()).astype(np.float16)).cuda()
        return net, hg, table
    net = api.Network(n_neurons=128, n_hidden_layers=8)
    net.set_params(torch.from_numpy(scenes.xavier_params_fp16(128, 8, net.encoded_width(), seed=1)).cuda())
    return net, None, None


def sphere(n):
    ax = torch.linspace(-1.0, 1.0, n, device="cuda")
    d2 = (ax * ax)[:, None, None] + (ax * ax)[None, :, None] + (ax * ax)[None, None, :]
    return (0.8 - d2.sqrt_()).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--lattices", default="128,256")
    ap.add_argument("--spheres", default="256,640")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_bench.py needs a GPU"
    print(f"# {torch.cuda.get_device_name(0)}; HIP events around each call, 1 warm-up + {args.runs} repetitions per row, rows alternating")

    print("\n## density_lattice (sigma of the model at n^3 nodes, one call, default runs_per_pass = 65536)")
    rows, info = [], {}
    keep = []
    for kind in ("hash", "freq"):
        net, hg, table = model(kind)
        keep.append((net, hg, table))
        for n in (int(v) for v in args.lattices.split(",")):
            out = torch.empty((n, n, n), device="cuda")
            ws = api.density_lattice_workspace((n, n, n), min(api.density_lattice_runs((n, n, n)), 1 << 16))
            name = f"{kind} {n}^3"
            rows.append((name, lambda net=net, hg=hg, table=table, n=n, out=out, ws=ws:
                         api.density_lattice(net, grid=hg, table=table, resolution=n, scale=1.0, out=out, workspace=ws)))
            info[name] = (n ** 3, RATES[kind])
    for name, ms in run_rows(rows, args.runs).items():
        samples, rate = info[name]
        med = statistics.median(ms)
        show(name, ms, f"   {samples / 1e6:.1f} M samples, {samples / med / 1e6:.2f} Gsamples/s; ideal {1e3 * samples / rate:.3f} ms "
                       f"at {rate / 1e9:.2f} Gsamples/s: {1e3 * samples / rate / med:.2f} of it")
    del rows, keep
    torch.cuda.empty_cache()

    print("\n## isosurface (analytic sphere, iso 0)")
    for n in (int(v) for v in args.spheres.split(",")):
        lattice = sphere(n)
        box = ((-1.0,) * 3, (1.0,) * 3)
        ws = api.isosurface_workspace((n, n, n))
        counts = torch.zeros(3, dtype=torch.int32, device="cuda")
        v, t, nrm, _ = api.isosurface(lattice, 0.0, box, normals=True, workspace=ws)
        V, T = v.shape[0], t.shape[0]
        nodes = n ** 3
        where = "inside the 256 MiB Infinity Cache" if nodes * 4 < (256 << 20) else "HBM"
        print(f"\n{n}^3 nodes = {nodes * 4 / 1e6:.0f} MB of lattice ({where}); {V} vertices, {T} triangles")
        from rtx_nerf_amd import _lib
        import ctypes as C

        def counts_only():
            a = _lib.IsosurfaceArgs()
            a.density, a.n = lattice.data_ptr(), (C.c_int * 3)(n, n, n)
            a.lo, a.hi, a.iso = (C.c_float * 3)(*box[0]), (C.c_float * 3)(*box[1]), 0.0
            a.counts, a.workspace, a.workspace_bytes = counts.data_ptr(), ws.data_ptr(), ws.numel() * 4
            _lib.check(_lib.lib().rtxn_isosurface(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rtxn_isosurface")

        def full(normals):
            api.isosurface(lattice, 0.0, box, normals=normals, max_vertices=V, max_triangles=T, counts=counts, vertices=v, triangles=t,
                           normals_out=nrm if normals else None, workspace=ws)

        times = run_rows([("counts only (count + scan)", counts_only), ("full, no normals", lambda: full(False)),
                          ("full, normals", lambda: full(True))], args.runs)
        b1 = nodes * 4
        med = {k: statistics.median(ms) for k, ms in times.items()}
        show("counts only (count + scan)", times["counts only (count + scan)"],
             f"   {b1 / 1e6:.0f} MB: {b1 / med['counts only (count + scan)'] / 1e6:.0f} GB/s = "
             f"{b1 / med['counts only (count + scan)'] * 1e3 / COPY_RATE:.2f} of the copy rate")
        for key, per_vertex in (("full, no normals", 12), ("full, normals", 24)):
            b2 = nodes * 4 + V * per_vertex + T * 12
            emit = med[key] - med["counts only (count + scan)"]
            show(key, times[key], f"   emit = {emit:.3f} ms for {b2 / 1e6:.0f} MB: {b2 / emit / 1e6:.0f} GB/s = {b2 / emit * 1e3 / COPY_RATE:.2f} "
                                  f"of the copy rate")
        del lattice, ws, v, t, nrm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
