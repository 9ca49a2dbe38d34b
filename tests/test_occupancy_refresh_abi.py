"""The device-side occupancy refresh (rtxn_occupancy_refresh and its two companions) at the C-ABI boundary, without a GPU:
the symbols exist, the ctypes struct mirrors the header, the workspace size behaves as include/rtxn.h says, and argument
errors come with their messages before any device is touched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["rtxn_occupancy_refresh_supported", "rtxn_occupancy_refresh_workspace_bytes", "rtxn_occupancy_refresh"]
FIELDS = ["mlp", "grid", "n_dir_freqs", "table_fp16", "grid_res",
          "density", "decay", "thickness_scale", "threshold", "threshold_mode",
          "jitter", "seed", "step",
          "occupancy", "coarse", "bricks", "super_mip",
          "occupied", "mean",
          "workspace", "workspace_bytes", "runs_per_pass"]


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def _header_fields(name):
    src = _header()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.split("{")[-1].strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())[0])
    return fields


def test_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", src), f"{n} is not declared in include/rtxn.h"
        assert hasattr(lib, n), f"{n} is not exported by librtxn.so"
        assert n in _lib.SYMBOLS
    assert "RTXN_OCC_ABSOLUTE = 0" in src and "RTXN_OCC_MIN_MEAN = 1" in src
    assert lib.rtxn_version() == 100


def test_struct_matches_the_header():
    from rtx_nerf_amd import _lib
    assert _header_fields("rtxn_occupancy_refresh_args") == FIELDS
    assert [f[0] for f in _lib.OccupancyRefreshArgs._fields_] == FIELDS
    # 13 pointers / size_t / long, 9 four-byte scalars of which n_dir_freqs and grid_res sit alone before a pointer
    assert C.sizeof(_lib.OccupancyRefreshArgs) == 152
    assert _lib.OccupancyRefreshArgs.density.offset == 40 and _lib.OccupancyRefreshArgs.step.offset == 72
    assert _lib.OccupancyRefreshArgs.runs_per_pass.offset == 144


def test_the_existing_structs_are_untouched():
    from rtx_nerf_amd import _lib
    assert hasattr(_lib, "OccupancyRefreshArgs")
    assert C.sizeof(_lib.RenderConfig) == 112 and C.sizeof(_lib.RenderStats) == 48 and C.sizeof(_lib.RenderOutputs) == 40
    assert C.sizeof(_lib.RenderTermination) == 12 and C.sizeof(_lib.RenderTerminationStats) == 40
    assert C.sizeof(_lib.TraceParams) == 232 and C.sizeof(_lib.TrainBackground) == 40
    assert C.sizeof(_lib.TrainBatch) == 240 and C.sizeof(_lib.TrainState) == 120 and C.sizeof(_lib.TrainStepArgs) == 608


def test_workspace_size():
    from rtx_nerf_amd import _lib
    wsb = _lib.lib().rtxn_occupancy_refresh_workspace_bytes
    err = _lib.lib().rtxn_last_error
    for R in (6, 20, 32, 48, 128):
        runs = R * R * ((R + 31) // 32)
        prev = 0
        for P in (1, 7, runs, runs + 100):
            b = wsb(R, P)
            # 12 + 12 + 8 B of segment records and 32 half4 of radiance per run of a pass, one float per run of the grid
            assert b % 256 == 0 and b >= P * (32 + 32 * 8) + runs * 4 and b < P * (32 + 32 * 8) + runs * 4 + 8 * 256
            assert b > prev
            prev = b
    for R, P, word in ((0, 4, b"grid_res"), (-3, 4, b"grid_res"), (1025, 4, b"grid_res"), (32, 0, b"runs_per_pass"), (32, -1, b"runs_per_pass")):
        assert wsb(R, P) == 0 and word in err(), (R, P)


def _models(lib, _lib):
    freq = C.c_void_p()
    assert lib.rtxn_mlp_create(C.byref(_lib.MlpConfig(3, 10, 2, 12, 64, 2, 4, 1)), C.byref(freq)) == 0
    ext = C.c_void_p()
    assert lib.rtxn_mlp_create(C.byref(_lib.MlpConfig(3, 10, 2, 4, 64, 4, 4, 1, 1, 32)), C.byref(ext)) == 0
    grid = C.c_void_p()        # 8 levels x 2 features + Frequency(4) on two angles = 32 wide: the fused hash kernel's kind
    assert lib.rtxn_hashgrid_create(C.byref(_lib.HashGridConfig(8, 2, 12, 4, 1.5)), C.byref(grid)) == 0
    odd = C.c_void_p()         # 4 features per level: rtxn_hashmlp_supported says no
    assert lib.rtxn_hashgrid_create(C.byref(_lib.HashGridConfig(2, 4, 12, 4, 1.5)), C.byref(odd)) == 0
    return freq, ext, grid, odd


def test_support_query():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    freq, ext, grid, odd = _models(lib, _lib)
    q = lib.rtxn_occupancy_refresh_supported
    assert q(freq, None, 0) == 1
    assert q(None, None, 0) == 0
    assert q(ext, None, 0) == 0                           # a pre-encoded model has no encoder of its own
    for g, df in ((grid, 4), (grid, 2), (odd, 4)):
        assert q(ext, g, df) == lib.rtxn_hashmlp_supported(ext, g, df)
    assert q(ext, grid, 4) == 1 and q(ext, odd, 4) == 0
    for h in (freq, ext):
        assert lib.rtxn_mlp_destroy(h) == 0
    for h in (grid, odd):
        assert lib.rtxn_hashgrid_destroy(h) == 0


def test_validation_precedes_device_use():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    freq, ext, grid, odd = _models(lib, _lib)
    call, err = lib.rtxn_occupancy_refresh, lib.rtxn_last_error
    R, P = 32, 64
    need = lib.rtxn_occupancy_refresh_workspace_bytes(R, P)
    fake = 0x10000                                        # never dereferenced: every case below stops before the device

    def args(**kw):
        a = _lib.OccupancyRefreshArgs()
        a.mlp, a.grid_res, a.density, a.decay, a.thickness_scale, a.threshold = freq, R, fake, 0.95, 2.0 / R, 0.01
        a.threshold_mode, a.occupancy, a.coarse, a.bricks, a.super_mip = 1, fake, fake, fake, fake
        a.workspace, a.workspace_bytes, a.runs_per_pass = fake, need, P
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [(dict(mlp=None), b"NULL model"), (dict(density=None), b"NULL density"),
           (dict(decay=-0.1), b"decay"), (dict(decay=1.5), b"decay"), (dict(decay=float("nan")), b"decay"),
           (dict(threshold_mode=2), b"unknown threshold mode"), (dict(threshold_mode=-1), b"unknown threshold mode"),
           (dict(workspace_bytes=need - 1), b"too small"), (dict(workspace=None), b"workspace"),
           (dict(runs_per_pass=0), b"runs_per_pass"), (dict(grid_res=0), b"grid_res"), (dict(occupancy=None), b"NULL occupancy"),
           (dict(grid_res=30, super_mip=None, workspace_bytes=1 << 30), b"coarse"),          # R % 4 != 0 with a 4^3 mip
           (dict(grid_res=20, workspace_bytes=1 << 30), b"super_mip"),                       # R % 16 != 0 with a 16^3 mip
           (dict(coarse=None), b"coarse"), (dict(bricks=None), b"bricks"),                   # R % 4 == 0: both are required
           (dict(mlp=ext, grid=grid, n_dir_freqs=4, table_fp16=None), b"table")]
    for kw, word in bad:
        a = args(**kw)
        assert call(C.byref(a), None) == 1 and word in err(), (kw, err())
    assert call(None, None) == 1 and b"NULL args" in err()
    # a valid request this build has no kernel for
    for kw in (dict(mlp=ext), dict(mlp=ext, grid=odd, n_dir_freqs=4, table_fp16=fake)):
        a = args(**kw)
        assert call(C.byref(a), None) == 3 and b"no fused inference kernel" in err(), kw
    # valid calls reach the device check: RTXN_ERR_HIP on a machine without one; with one, these models have no parameters
    # yet, which is the first thing looked at behind that check (still nothing is launched)
    import torch
    want = (1, b"rtxn_mlp_set_params") if torch.cuda.is_available() else (2, b"no HIP device")
    for kw in (dict(), dict(mlp=ext, grid=grid, n_dir_freqs=4, table_fp16=fake),
               dict(grid_res=6, coarse=None, bricks=None, super_mip=None, workspace_bytes=1 << 30)):
        a = args(**kw)
        assert call(C.byref(a), None) == want[0] and want[1] in err(), (kw, err())
    for h in (freq, ext):
        assert lib.rtxn_mlp_destroy(h) == 0
    for h in (grid, odd):
        assert lib.rtxn_hashgrid_destroy(h) == 0
