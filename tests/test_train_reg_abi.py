"""CPU-side checks of the distortion regulariser at the C-ABI boundary (rtxn_train_regularizer, rtxn_volrender_reg_train,
rtxn_train_gradients_reg, rtxn_train_step_reg): symbols and bindings, the struct's layout against the C compiler,
and the rules every entry point checks before any device is touched.  The Trainer's own refusals are checked here too (they
raise before allocating)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_volrender_reg_train", "rtxn_train_gradients_reg", "rtxn_train_step_reg")
VR_COMPAT, VR_NERF = 0, 1
REGULAR, MIDPOINT_WORLD, JITTER_WORLD = 0, 3, 4
TRACE_COMPAT, TRACE_DDA = 0, 1
P = C.c_void_p(4096)           # a fake device pointer: never launched from here
FIELDS = ["distortion_weight", "t_start", "t_end", "distortion", "depth"]


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_regularizer_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    assert lib.rtxn_version() == 100


def test_train_regularizer_layout_matches_the_header_and_the_c_compiler(tmp_path):
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index("typedef struct rtxn_train_regularizer {"):src.index("} rtxn_train_regularizer;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = [re.findall(r"([A-Za-z_]\w*)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    T = _lib.TrainRegularizer
    assert fields == [f[0] for f in T._fields_] == FIELDS
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                 "sizeof(rtxn_train_regularizer), " + ", ".join(f"offsetof(rtxn_train_regularizer, {f})" for f in FIELDS)
                 + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(c), "-o", str(exe)])
    want = [C.sizeof(T)] + [getattr(T, f).offset for f in FIELDS]
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == want == [40, 0, 8, 16, 24, 32]


def _reg(_lib, weight=0.5, t_start=P, t_end=P, distortion=None, depth=None):
    s = _lib.TrainRegularizer()
    s.distortion_weight, s.t_start, s.t_end, s.distortion, s.depth = weight, t_start, t_end, distortion, depth
    return s


def _entries(_lib, reg, vr=VR_NERF, stype=MIDPOINT_WORLD, trace=TRACE_DDA):
    """(name, return code, message) of the three entry points on an otherwise empty batch: an accepted spec fails later, on the
    batch's own checks, under the entry point it forwards to"""
    lib = _lib.lib()
    batch = _lib.TrainBatch()
    batch.vr_mode, batch.sample_type = vr, stype
    args = _lib.TrainStepArgs()
    args.batch.vr_mode, args.batch.sample_type, args.trace.mode = vr, stype, trace
    jit = _lib.SampleJitter() if stype == JITTER_WORLD else None
    jp = C.byref(jit) if jit is not None else None
    rp = C.byref(reg) if reg is not None else None
    out = [("rtxn_train_gradients_reg", lib.rtxn_train_gradients_reg(C.byref(batch), None, jp, None, rp, None), lib.rtxn_last_error()),
           ("rtxn_train_step_reg", lib.rtxn_train_step_reg(C.byref(args), None, jp, None, rp, None), lib.rtxn_last_error())]
    if vr == VR_NERF:                    # the compositor has no mode argument: it is the NeRF one
        out.append(("rtxn_volrender_reg_train", lib.rtxn_volrender_reg_train(P, P, P, P, 4, 32, P, 128.0, P, P, P, P, None, None, rp, None),
                    lib.rtxn_last_error()))
    return out


# (weight, t_start, t_end, distortion, depth) -> the field the message names
_REJECTED = [((-0.5, P, P, None, None), b"reg->distortion_weight"), ((float("nan"), P, P, None, None), b"reg->distortion_weight"),
             ((float("inf"), P, P, None, None), b"reg->distortion_weight"), ((-1.0, None, None, None, None), b"reg->distortion_weight"),
             ((0.5, None, P, None, None), b"reg->t_start"), ((0.5, P, None, None, None), b"reg->t_end"),
             ((0.5, None, None, None, None), b"reg->t_start"),
             ((0.0, None, None, P, None), b"reg->t_start"), ((0.0, None, P, None, P), b"reg->t_start")]


@pytest.mark.parametrize("case,word", _REJECTED)
def test_reg_entries_reject_bad_specs_before_touching_a_device(case, word):
    """RTXN_ERR_INVALID (1) and a message naming the field, with or without a GPU; the buffers are never looked at."""
    from rtx_nerf_amd import _lib
    for name, rc, msg in _entries(_lib, _reg(_lib, *case)):
        assert rc == 1 and word in msg and name.encode() in msg, (name, rc, msg)


@pytest.mark.parametrize("reg_kw", [dict(weight=0.5), dict(weight=0.0, distortion=P), dict(weight=0.0, depth=P)])
def test_reg_needs_the_nerf_compositor_world_samples_and_the_dda_walk(reg_kw):
    from rtx_nerf_amd import _lib
    for name, rc, msg in _entries(_lib, _reg(_lib, **reg_kw), vr=VR_COMPAT, stype=REGULAR):
        assert rc == 1 and b"RTXN_VR_NERF" in msg and b"reg->distortion_weight" in msg and name.encode() in msg, (name, msg)
    for name, rc, msg in _entries(_lib, _reg(_lib, **reg_kw), stype=REGULAR):
        if name != "rtxn_volrender_reg_train":           # the compositor has no sample type
            assert rc == 1 and b"sample_type" in msg and b"RTXN_SAMPLING_MIDPOINT_WORLD" in msg and name.encode() in msg, (name, msg)
    for stype in (MIDPOINT_WORLD, JITTER_WORLD):
        for name, rc, msg in _entries(_lib, _reg(_lib, **reg_kw), stype=stype, trace=TRACE_COMPAT):
            if name == "rtxn_train_step_reg":
                assert rc == 1 and b"trace.mode" in msg and b"RTXN_TRACE_COMPAT" in msg and b"rtxn_train_step_reg" in msg, msg
            elif name == "rtxn_train_gradients_reg":     # accepted: the batch's own checks, under the name they carry
                assert rc == 1 and b"NULL batch or model" in msg, msg


def test_valid_and_inactive_specs_reach_the_device_check_or_the_plain_checks():
    """A valid spec passes the rules: the compositor then needs a device (RTXN_ERR_HIP = 2 without one; with one, an empty batch
    is RTXN_OK and touches no buffer), the batch entry points meet the batch's own checks.  NULL, or weight 0 without outputs,
    is the _loss call: the existing entry points' own checks, under their names, whatever the mode."""
    import torch
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    want = 0 if torch.cuda.is_available() else 2
    for reg in (_reg(_lib, 0.5), _reg(_lib, 0.5, distortion=P, depth=P), _reg(_lib, 0.0, depth=P)):
        assert lib.rtxn_volrender_reg_train(P, P, P, P, 0, 32, P, 128.0, P, P, None, P, None, None, C.byref(reg), None) == want
        if want == 2:
            assert b"no HIP device" in lib.rtxn_last_error()
        assert lib.rtxn_volrender_reg_train(P, P, P, P, -1, 32, P, 1.0, P, P, P, P, None, None, C.byref(reg), None) == 1
        assert b"rtxn_volrender_reg_train: batch_size" in lib.rtxn_last_error()
        for stype in (MIDPOINT_WORLD, JITTER_WORLD):
            for name, rc, msg in _entries(_lib, reg, stype=stype)[:2]:
                assert rc == 1 and (b"NULL batch or model" in msg or b"batch.mlp is NULL" in msg), (name, msg)
    for reg in (None, _reg(_lib, 0.0, None, None)):
        rp = C.byref(reg) if reg is not None else None
        assert lib.rtxn_volrender_reg_train(P, P, P, P, -1, 32, P, 1.0, P, P, P, P, None, None, rp, None) == 1
        assert b"rtxn_volrender_l2_train: batch_size" in lib.rtxn_last_error()
        for name, rc, msg in _entries(_lib, reg, vr=VR_COMPAT, stype=REGULAR, trace=TRACE_COMPAT)[:2]:
            assert rc == 1 and (b"NULL batch or model" in msg or b"batch.mlp is NULL" in msg), (name, msg)
    assert lib.rtxn_train_gradients_reg(None, None, None, None, None, None) == 1 and b"NULL batch" in lib.rtxn_last_error()
    assert lib.rtxn_train_step_reg(None, None, None, None, None, None) == 1 and b"NULL arguments" in lib.rtxn_last_error()


def test_train_regularizer_struct_from_python():
    from rtx_nerf_amd import api
    s = api.train_regularizer()
    assert s.distortion_weight == 0.0 and not s.t_start and not s.t_end and not s.distortion and not s.depth
    assert api.train_regularizer(0.25).distortion_weight == 0.25
    import inspect
    assert "regularizer" in inspect.signature(api.train_gradients).parameters
    assert "regularizer" in inspect.signature(api.train_step).parameters
    assert "regularizer" in inspect.signature(api.volrender_reg_train).parameters


@pytest.mark.parametrize("kw,word", [(dict(distortion_weight=-1.0), "distortion_weight = -1.0"),
                                     (dict(distortion_weight=float("nan")), "distortion_weight"),
                                     (dict(distortion_weight=0.01, mode="compat"), "mode='nerf'")])
def test_trainer_refuses_regularisers_it_cannot_train(kw, word):
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match=re.escape(word)):
        Trainer(16, None, encoding="freq", device="cpu", **kw)


def test_trainer_refuses_the_regulariser_with_the_three_launch_compositor(monkeypatch):
    from rtx_nerf_amd.train import Trainer
    monkeypatch.setenv("RTXN_TRAIN_FUSE_COMPOSITOR", "0")
    with pytest.raises(ValueError, match="RTXN_TRAIN_FUSE_COMPOSITOR=0"):
        Trainer(16, None, encoding="freq", device="cpu", distortion_weight=0.01)
