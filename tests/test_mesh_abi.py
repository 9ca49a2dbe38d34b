"""Mesh extraction (rtxn_density_lattice, rtxn_isosurface and their workspace queries) at the C-ABI boundary, without a GPU: the
symbols exist, the ctypes structs mirror the header, the workspace sizes behave as include/rtxn.h says, and argument errors come
with a message naming the field before any device is touched.  The pattern of test_occupancy_refresh_abi.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["rtxn_density_lattice_workspace_bytes", "rtxn_density_lattice", "rtxn_isosurface_workspace_bytes", "rtxn_isosurface"]
LATTICE_FIELDS = ["mlp", "grid", "n_dir_freqs", "table_fp16", "n", "lo", "hi", "scale", "density", "workspace", "workspace_bytes",
                  "runs_per_pass"]
ISO_FIELDS = ["density", "n", "lo", "hi", "iso", "vertices", "normals", "triangles", "max_vertices", "max_triangles", "counts",
              "workspace", "workspace_bytes"]


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def _header_fields(name):
    src = _header()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.split("{")[-1].strip()
        if decl:
            fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?$", decl)[0])
    return fields


def _n(*v):
    return (C.c_int * 3)(*v)


def test_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib, api
    from rtx_nerf_amd.train import Trainer
    lib = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", src), f"{n} is not declared in include/rtxn.h"
        assert hasattr(lib, n), f"{n} is not exported by librtxn.so"
        assert n in _lib.SYMBOLS
    for fn in ("density_lattice", "isosurface", "write_ply", "density_lattice_workspace", "isosurface_workspace"):
        assert callable(getattr(api, fn))
    assert callable(Trainer.extract_mesh)
    assert lib.rtxn_version() == 100


def test_structs_match_the_header():
    from rtx_nerf_amd import _lib
    assert _header_fields("rtxn_density_lattice_args") == LATTICE_FIELDS
    assert [f[0] for f in _lib.DensityLatticeArgs._fields_] == LATTICE_FIELDS
    assert _header_fields("rtxn_isosurface_args") == ISO_FIELDS
    assert [f[0] for f in _lib.IsosurfaceArgs._fields_] == ISO_FIELDS
    L, S = _lib.DensityLatticeArgs, _lib.IsosurfaceArgs
    # lattice: 3 pointers and an int before n (32), ten 4-byte scalars (n, lo, hi, scale) to 72, then four 8-byte fields
    assert C.sizeof(L) == 104 and L.n.offset == 32 and L.scale.offset == 68 and L.density.offset == 72 and L.runs_per_pass.offset == 96
    # isosurface: a pointer, ten 4-byte scalars (n, lo, hi, iso) to 48, three pointers, two ints, three 8-byte fields
    assert C.sizeof(S) == 104 and S.n.offset == 8 and S.iso.offset == 44 and S.vertices.offset == 48 and S.max_vertices.offset == 72
    assert S.counts.offset == 80 and S.workspace_bytes.offset == 96


def test_the_existing_structs_are_untouched():
    from rtx_nerf_amd import _lib
    assert C.sizeof(_lib.OccupancyRefreshArgs) == 152 and C.sizeof(_lib.RenderConfig) == 112
    assert C.sizeof(_lib.TrainBatch) == 240 and C.sizeof(_lib.TrainStepArgs) == 608 and C.sizeof(_lib.ImageMetricsArgs) == 104


def test_workspace_sizes():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    lat, iso, err = lib.rtxn_density_lattice_workspace_bytes, lib.rtxn_isosurface_workspace_bytes, lib.rtxn_last_error
    for n in ((2, 2, 2), (5, 4, 33), (128, 128, 128), (1024, 3, 70)):
        prev = 0
        for P in (1, 7, 4096):
            b = lat(_n(*n), P)
            # 12 + 12 + 8 B of segment records and 32 half4 of radiance per run of a pass: the lattice's size does not enter
            assert b % 256 == 0 and P * (32 + 32 * 8) <= b < P * (32 + 32 * 8) + 6 * 256 and b > prev
            assert b == lat(_n(2, 2, 2), P)
            prev = b
        rows, nodes = n[0] * n[1], n[0] * n[1] * n[2]
        b = iso(_n(*n))
        # one word per node; two counts and two offsets per row (x, y); four 64-bit words per group of 1024 rows, 1024 groups
        assert b % 256 == 0 and nodes * 4 + rows * 16 + 32768 <= b < nodes * 4 + rows * 16 + 32768 + 6 * 256
    for n, P, word in (((1, 4, 4), 4, b"n[0]"), ((4, 1025, 4), 4, b"n[1]"), ((4, 4, 0), 4, b"n[2]"), ((4, 4, 4), 0, b"runs_per_pass"),
                       ((4, 4, 4), -1, b"runs_per_pass")):
        assert lat(_n(*n), P) == 0 and word in err(), (n, P)
    for n, word in (((1, 4, 4), b"n[0]"), ((4, 4, 1025), b"n[2]")):
        assert iso(_n(*n)) == 0 and word in err(), n
    assert lat(None, 4) == 0 and b"NULL n" in err()
    assert iso(None) == 0 and b"NULL n" in err()


def _models(lib, _lib):
    freq = C.c_void_p()
    assert lib.rtxn_mlp_create(C.byref(_lib.MlpConfig(3, 10, 2, 12, 64, 2, 4, 1)), C.byref(freq)) == 0
    ext = C.c_void_p()
    assert lib.rtxn_mlp_create(C.byref(_lib.MlpConfig(3, 10, 2, 4, 64, 4, 4, 1, 1, 32)), C.byref(ext)) == 0
    grid = C.c_void_p()
    assert lib.rtxn_hashgrid_create(C.byref(_lib.HashGridConfig(8, 2, 12, 4, 1.5)), C.byref(grid)) == 0
    odd = C.c_void_p()         # 4 features per level: rtxn_hashmlp_supported says no
    assert lib.rtxn_hashgrid_create(C.byref(_lib.HashGridConfig(2, 4, 12, 4, 1.5)), C.byref(odd)) == 0
    return freq, ext, grid, odd


def test_lattice_validation_precedes_device_use():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    freq, ext, grid, odd = _models(lib, _lib)
    call, err = lib.rtxn_density_lattice, lib.rtxn_last_error
    P = 16
    need = lib.rtxn_density_lattice_workspace_bytes(_n(5, 4, 33), P)
    fake = 0x10000                                        # never dereferenced: every case below stops before the device

    def args(**kw):
        a = _lib.DensityLatticeArgs()
        a.mlp, a.n, a.lo, a.hi, a.scale = freq, _n(5, 4, 33), (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1), 37.0
        a.density, a.workspace, a.workspace_bytes, a.runs_per_pass = fake, fake, need, P
        for k, v in kw.items():
            setattr(a, k, (C.c_float * 3)(*v) if k in ("lo", "hi") else _n(*v) if k == "n" else v)
        return a

    bad = [(dict(mlp=None), b"NULL model"), (dict(n=(1, 4, 4)), b"n[0]"), (dict(n=(4, 4, 1025)), b"n[2]"),
           (dict(lo=(-1, 0.5, -1), hi=(1, 0.5, 1)), b"lo < hi"), (dict(lo=(-1, -1, 0.7), hi=(1, 1, 0.2)), b"lo < hi"),
           (dict(lo=(float("nan"), -1, -1)), b"lo < hi"), (dict(hi=(1, 1.5, 1)), b"[-1,1]"), (dict(lo=(-1.01, -1, -1)), b"[-1,1]"),
           (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"), (dict(density=None), b"NULL density"),
           (dict(workspace_bytes=need - 1), b"too small"), (dict(workspace=None), b"workspace"), (dict(workspace=fake + 4), b"aligned"),
           (dict(runs_per_pass=0), b"runs_per_pass"), (dict(mlp=ext, grid=grid, n_dir_freqs=4, table_fp16=None), b"table")]
    for kw, word in bad:
        assert call(C.byref(args(**kw)), None) == 1 and word in err(), (kw, err())
    assert call(None, None) == 1 and b"NULL args" in err()
    # the support rule is the refresh's: a valid request this build has no kernel for
    for kw in (dict(mlp=ext), dict(mlp=ext, grid=odd, n_dir_freqs=4, table_fp16=fake)):
        assert lib.rtxn_occupancy_refresh_supported(kw["mlp"], kw.get("grid"), kw.get("n_dir_freqs", 0)) == 0
        assert call(C.byref(args(**kw)), None) == 3 and b"no fused inference kernel" in err(), kw
    # valid calls reach the device check: RTXN_ERR_HIP on a machine without one; with one, these models have no parameters yet
    import torch
    want = (1, b"rtxn_mlp_set_params") if torch.cuda.is_available() else (2, b"no HIP device")
    for kw in (dict(), dict(mlp=ext, grid=grid, n_dir_freqs=4, table_fp16=fake)):
        assert call(C.byref(args(**kw)), None) == want[0] and want[1] in err(), (kw, err())
    for h in (freq, ext):
        assert lib.rtxn_mlp_destroy(h) == 0
    for h in (grid, odd):
        assert lib.rtxn_hashgrid_destroy(h) == 0


def test_isosurface_validation_precedes_device_use():
    import torch
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    call, err = lib.rtxn_isosurface, lib.rtxn_last_error
    need = lib.rtxn_isosurface_workspace_bytes(_n(6, 7, 8))
    fake = 0x10000

    def args(**kw):
        a = _lib.IsosurfaceArgs()
        a.density, a.n, a.lo, a.hi, a.iso = fake, _n(6, 7, 8), (C.c_float * 3)(-0.7, -1, -0.31), (C.c_float * 3)(0.9, 0.55, 1), 0.37
        a.vertices, a.normals, a.triangles, a.max_vertices, a.max_triangles, a.counts = fake, fake, fake, 100, 200, fake
        a.workspace, a.workspace_bytes = fake, need
        for k, v in kw.items():
            setattr(a, k, (C.c_float * 3)(*v) if k in ("lo", "hi") else _n(*v) if k == "n" else v)
        return a

    bad = [(dict(density=None), b"NULL density"), (dict(n=(6, 1, 8)), b"n[1]"), (dict(n=(1025, 7, 8)), b"n[0]"),
           (dict(lo=(0.9, -1, -0.31)), b"lo < hi"), (dict(hi=(0.9, float("inf"), 1)), b"lo < hi"),
           (dict(iso=float("nan")), b"iso"), (dict(iso=float("-inf")), b"iso"), (dict(max_vertices=-1), b"max_vertices"),
           (dict(max_triangles=-5), b"max_triangles"), (dict(vertices=None), b"normals without vertices"),
           (dict(counts=None), b"NULL counts"), (dict(workspace=None), b"workspace"), (dict(workspace=fake + 8), b"aligned"),
           (dict(workspace_bytes=need - 1), b"too small")]
    for kw, word in bad:
        assert call(C.byref(args(**kw)), None) == 1 and word in err(), (kw, err())
    assert call(None, None) == 1 and b"NULL args" in err()
    # a box outside the cube is the isosurface's to take: any lattice, not only rtxn_density_lattice's
    # (with a device these valid calls would run on the fake pointers: test_gpu_isosurface.py makes them on real ones)
    if not torch.cuda.is_available():
        for kw in (dict(), dict(vertices=None, normals=None, triangles=None), dict(lo=(-5, -5, -5), hi=(7, 8, 9))):
            assert call(C.byref(args(**kw)), None) == 2 and b"no HIP device" in err(), (kw, err())
