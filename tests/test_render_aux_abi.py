"""CPU-side checks of the depth / opacity / background outputs at the C-ABI boundary (rtxn_volrender_fwd_aux,
RTXN_RENDER_AUX, rtxn_render_outputs, rtxn_render_frame[_async]_ex): symbols and bindings, the workspace the flag adds, and
argument validation that happens before any device is touched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_volrender_fwd_aux", "rtxn_render_frame_ex", "rtxn_render_frame_async_ex")
RENDER_AUX = 4


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_aux_symbols_are_exported_and_bound():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    assert lib.rtxn_version() == 100


def test_render_outputs_matches_header_order():
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index("typedef struct rtxn_render_outputs {"):src.index("} rtxn_render_outputs;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = [re.findall(r"([A-Za-z_]\w*)\s*(?:\[\d+\])?\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.RenderOutputs._fields_] == ["pixels", "depth", "opacity", "background"]
    assert C.sizeof(_lib.RenderOutputs) == 3 * C.sizeof(C.c_void_p) + 3 * 4 + 4      # three floats of background, padded to 8
    assert re.search(r"RTXN_RENDER_AUX\s*=\s*4\b", src)


def _config(lib, _lib, h, **kw):
    rc = _lib.RenderConfig()
    rc.mlp, rc.width, rc.height, rc.grid_res, rc.trace_mode, rc.max_segments, rc.n_slots = h, 64, 48, 32, 1, 1000, 3
    rc.focal_length, rc.aspect_ratio = 1.0, 64 / 48
    for k, v in kw.items():
        setattr(rc, k, v)
    return rc


def test_aux_flag_grows_the_workspace_only_when_set():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    cfg = _lib.MlpConfig(3, 10, 2, 12, 64, 2, 4, 1)
    h = C.c_void_p()
    assert lib.rtxn_mlp_create(C.byref(cfg), C.byref(h)) == 0
    try:
        # byte counts of the parent revision for these configs: a renderer without the flag lays out exactly what it did
        for kw, before in ((dict(), 1_052_160), (dict(flags=1), 2_204_160), (dict(n_slots=1, max_segments=4321), 1_307_392)):
            rc = _config(lib, _lib, h, **kw)
            plain = lib.rtxn_render_workspace_bytes(C.byref(rc))
            assert plain == before, (kw, plain)
            rc.flags |= RENDER_AUX
            aux = lib.rtxn_render_workspace_bytes(C.byref(rc))
            assert aux >= plain + rc.n_slots * rc.max_segments * 8, (kw, plain, aux)
            assert aux <= plain + rc.n_slots * (rc.max_segments * 8 + 2 * 256)       # t_start + t_end per slot, nothing else
            assert aux % 256 == 0
        rc = _config(lib, _lib, h, flags=RENDER_AUX, trace_mode=0)   # RTXN_TRACE_COMPAT: t from re-launched origins
        assert lib.rtxn_render_workspace_bytes(C.byref(rc)) == 0 and b"RTXN_TRACE_DDA" in lib.rtxn_last_error()
        rc = _config(lib, _lib, h, flags=8)
        assert lib.rtxn_render_workspace_bytes(C.byref(rc)) == 0 and b"unknown flags" in lib.rtxn_last_error()
    finally:
        assert lib.rtxn_mlp_destroy(h) == 0


def test_aux_entries_validate_before_touching_a_device():
    """Argument errors are RTXN_ERR_INVALID with a message, with or without a GPU."""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    out = _lib.RenderOutputs()
    out.pixels = C.c_void_p(256)
    out.depth = C.c_void_p(512)
    la = (C.c_float * 16)()
    assert lib.rtxn_render_frame_ex(None, 0, C.cast(la, C.c_void_p), 0, 0, C.byref(out), None) == 1
    assert b"NULL argument" in lib.rtxn_last_error()
    assert lib.rtxn_render_frame_async_ex(None, C.cast(la, C.c_void_p), 1, 0, 0, C.byref(out), None, None) == 1
    assert b"NULL argument" in lib.rtxn_last_error()
    P = C.c_void_p(4096)
    bg = (C.c_float * 3)(1.0, 1.0, 1.0)
    # depth without the segment distances
    assert lib.rtxn_volrender_fwd_aux(P, 1, None, P, P, None, None, 4, 32, 0, 0, C.cast(bg, C.c_void_p), P, P, P, None) == 1
    assert b"t_start" in lib.rtxn_last_error()
    assert lib.rtxn_volrender_fwd_aux(P, 2, None, P, P, None, None, 4, 32, 0, 0, None, P, None, P, None) == 1
    assert b"layout" in lib.rtxn_last_error()
    assert lib.rtxn_volrender_fwd_aux(P, 1, None, P, P, None, None, 4, 32, 0, 1, None, P, None, P, None) == 1
    assert b"sample_type" in lib.rtxn_last_error()
    assert lib.rtxn_volrender_fwd_aux(P, 0, P, P, P, None, None, 4, 32, 2, 0, None, P, None, P, None) == 1
    assert b"mode" in lib.rtxn_last_error()
    assert lib.rtxn_volrender_fwd_aux(P, 0, P, P, P, None, None, -1, 32, 0, 0, None, P, None, P, None) == 1
    assert b"batch_size" in lib.rtxn_last_error()
