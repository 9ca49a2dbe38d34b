"""Early termination of the frame entry (rtxn_render_set_termination and its companions) at the C-ABI boundary, without a
GPU: the symbols exist, the ctypes structs mirror the header, argument errors come with their messages before any device
is touched, and the second workspace's size behaves as include/rtxn.h says."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["rtxn_render_termination_workspace_bytes", "rtxn_render_set_termination", "rtxn_render_termination_status",
               "rtxn_render_termination_buffers"]


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
    assert "#define RTXN_RENDER_MAX_ROUNDS 8" in _header()
    assert lib.rtxn_version() == 100


@pytest.mark.parametrize("c_name,binding,size", [("rtxn_render_termination", "RenderTermination", 12),
                                                 ("rtxn_render_termination_stats", "RenderTerminationStats", 40)])
def test_structs_match_the_header(c_name, binding, size):
    from rtx_nerf_amd import _lib
    assert _header_fields(c_name) == [f[0] for f in getattr(_lib, binding)._fields_]
    assert C.sizeof(getattr(_lib, binding)) == size


def test_the_existing_structs_and_flags_are_untouched():
    from rtx_nerf_amd import _lib
    assert _header_fields("rtxn_render_config")[-3:] == ["max_segments", "n_slots", "flags"] and C.sizeof(_lib.RenderConfig) == 112
    assert C.sizeof(_lib.RenderStats) == 48 and C.sizeof(_lib.RenderOutputs) == 40


def _config(lib, _lib):
    cfg = _lib.MlpConfig(3, 10, 2, 12, 64, 2, 4, 1)
    h = C.c_void_p()
    assert lib.rtxn_mlp_create(C.byref(cfg), C.byref(h)) == 0
    rc = _lib.RenderConfig()
    rc.mlp, rc.width, rc.height, rc.grid_res, rc.trace_mode, rc.max_segments, rc.n_slots = h, 64, 48, 32, 1, 1000, 1
    rc.focal_length, rc.aspect_ratio = 1.0, 64 / 48
    return h, rc


def test_validation_precedes_device_use():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    h, rc = _config(lib, _lib)
    wsb, setter = lib.rtxn_render_termination_workspace_bytes, lib.rtxn_render_set_termination
    bad = [((0.0, 4, 5), b"min_transmittance"), ((1.0, 4, 5), b"min_transmittance"), ((-0.1, 4, 5), b"min_transmittance"),
           ((float("nan"), 4, 5), b"min_transmittance"), ((1e-3, 0, 5), b"first_round_segments"), ((1e-3, -2, 5), b"first_round_segments"),
           ((1e-3, 4, 0), b"n_rounds"), ((1e-3, 4, 9), b"n_rounds")]
    for args, word in bad:
        t = _lib.RenderTermination(*args)
        assert wsb(C.byref(rc), C.byref(t)) == 0 and word in lib.rtxn_last_error(), args
        # the setter checks the termination before it looks at the renderer: RTXN_ERR_INVALID with the same message, no device
        assert setter(None, C.byref(t), None, 0) == 1 and word in lib.rtxn_last_error(), args
    good = _lib.RenderTermination(1e-3, 4, 5)
    assert setter(None, C.byref(good), None, 0) == 1 and b"NULL renderer" in lib.rtxn_last_error()
    assert setter(None, None, None, 0) == 1 and b"NULL renderer" in lib.rtxn_last_error()
    assert wsb(C.byref(rc), None) == 0 and b"NULL termination" in lib.rtxn_last_error()
    assert wsb(None, C.byref(good)) == 0 and b"NULL config" in lib.rtxn_last_error()
    st = _lib.RenderTerminationStats()
    assert lib.rtxn_render_termination_status(None, 0, C.byref(st)) == 1
    assert lib.rtxn_render_termination_buffers(None, 0, None) == 1
    # the float4 hand-over is out of scope, and flag bit 8 is still nobody's
    rc.flags = 1
    assert wsb(C.byref(rc), C.byref(good)) == 0 and b"RTXN_RENDER_FLOAT4" in lib.rtxn_last_error()
    rc.flags = 8
    assert wsb(C.byref(rc), C.byref(good)) == 0 and b"unknown flags" in lib.rtxn_last_error()
    assert lib.rtxn_render_workspace_bytes(C.byref(rc)) == 0 and b"unknown flags" in lib.rtxn_last_error()
    assert lib.rtxn_mlp_destroy(h) == 0


def test_workspace_size():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    h, rc = _config(lib, _lib)
    wsb = lib.rtxn_render_termination_workspace_bytes
    t = _lib.RenderTermination(1e-3, 4, 5)
    one = wsb(C.byref(rc), C.byref(t))
    m, n, K = 1000, 64 * 48, 32
    # one round's packed scratch at capacity (12 + 12 + 8 B records, half4 radiance) and 44 B of per-ray state
    assert one % 256 == 0 and one >= m * (32 + K * 8) + n * 44
    assert one < m * (32 + K * 8) + n * 44 + 64 * 1024
    # the schedule does not change the size: the scratch holds any one round
    assert wsb(C.byref(rc), C.byref(_lib.RenderTermination(0.5, 1, 8))) == one
    rc.trace_mode, rc.flags = 1, 4                          # RTXN_RENDER_AUX: + t_start / t_end per segment of capacity
    aux = wsb(C.byref(rc), C.byref(t))
    assert aux % 256 == 0 and aux >= one + 8 * m and aux <= one + 8 * m + 512
    rc.flags = 0
    for slots in (2, 3, 4):
        rc.n_slots = slots
        assert wsb(C.byref(rc), C.byref(t)) == slots * one
    assert lib.rtxn_mlp_destroy(h) == 0
