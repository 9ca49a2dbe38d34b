"""CPU-side checks of the sample jitter at the C-ABI boundary (RTXN_SAMPLING_JITTER_WORLD, rtxn_sample_jitter, the `_jitter`
entry points and rtxn_sample_ex): symbols and bindings, the struct's layout, and the three rules every new entry checks before any
device is touched.  The Trainer's own refusal is checked here too (it raises before allocating)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENT_ENTRIES = ("rtxn_encode_frequency_segments", "rtxn_hashgrid_encode_segments", "rtxn_mlp_train_forward_lean_segments",
                   "rtxn_mlp_train_backward_lean_segments", "rtxn_hashgrid_backward_segments", "rtxn_hashgrid_backward_segments_live")
NEW_SYMBOLS = tuple(n + "_jitter" for n in SEGMENT_ENTRIES) + ("rtxn_train_gradients_jitter", "rtxn_train_step_jitter", "rtxn_sample_ex")
REGULAR, MIDPOINT_WORLD, JITTER_WORLD = 0, 3, 4
VR_COMPAT, VR_NERF = 0, 1


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_jitter_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    for n in SEGMENT_ENTRIES:            # the new form is the old one plus the struct in front of the stream
        old, new = _lib.SYMBOLS[n][1], _lib.SYMBOLS[n + "_jitter"][1]
        assert new == old[:-1] + [C.POINTER(_lib.SampleJitter)] + old[-1:]
    assert lib.rtxn_version() == 100


def test_sample_jitter_matches_header_order_and_enum():
    from rtx_nerf_amd import _lib, api
    src = _header()
    body = src[src.index("typedef struct rtxn_sample_jitter {"):src.index("} rtxn_sample_jitter;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = [re.findall(r"([A-Za-z_]\w*)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.SampleJitter._fields_] == ["seed", "step"]
    assert C.sizeof(_lib.SampleJitter) == 16 and _lib.SampleJitter.seed.offset == 0 and _lib.SampleJitter.step.offset == 8
    assert re.search(r"RTXN_SAMPLING_JITTER_WORLD\s*=\s*4\b", src)
    assert re.search(r"RTXN_SAMPLING_MIDPOINT_WORLD\s*=\s*3\b", src)
    assert api.SAMPLING_JITTER_WORLD == 4
    j = api.sample_jitter(seed=-1)
    assert j.seed == 0xFFFFFFFF and not j.step


def _jit(_lib, seed=7):
    j = _lib.SampleJitter()
    j.seed = seed
    return j


def _call(lib, _lib, name, sample_type, jitter):
    """`name` with NULL buffers, the given sampling type and jitter (None: NULL); the status."""
    j = C.byref(jitter) if jitter is not None else None
    if name == "rtxn_encode_frequency_segments_jitter":
        return getattr(lib, name)(None, None, None, None, 4, sample_type, 1.0, None, None, j, None)
    if name == "rtxn_hashgrid_encode_segments_jitter":
        return getattr(lib, name)(None, 4, None, None, None, None, 4, sample_type, 1.0, None, None, j, None)
    if name == "rtxn_mlp_train_forward_lean_segments_jitter":
        return getattr(lib, name)(None, None, None, None, 4, sample_type, 1.0, None, None, None, None, j, None)
    if name == "rtxn_mlp_train_backward_lean_segments_jitter":
        return getattr(lib, name)(None, None, None, None, 4, sample_type, None, None, None, None, None, j, None)
    if name == "rtxn_hashgrid_backward_segments_jitter":
        return getattr(lib, name)(None, None, None, 4, sample_type, None, None, None, j, None)
    if name == "rtxn_hashgrid_backward_segments_live_jitter":
        return getattr(lib, name)(None, None, None, 4, sample_type, None, None, None, None, j, None)
    if name == "rtxn_sample_ex":
        return getattr(lib, name)(None, None, None, None, None, 4, 16, None, None, sample_type, j, None)
    raise AssertionError(name)


@pytest.mark.parametrize("name", [n for n in NEW_SYMBOLS if n not in ("rtxn_train_gradients_jitter", "rtxn_train_step_jitter")])
def test_segment_entries_check_the_jitter_before_touching_a_device(name):
    """RTXN_ERR_INVALID (1) and a message that names the entry, with or without a GPU; no buffer is looked at."""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert _call(lib, _lib, name, JITTER_WORLD, None) == 1
    assert b"needs a jitter struct" in lib.rtxn_last_error() and name.encode() in lib.rtxn_last_error()
    for st in (REGULAR, MIDPOINT_WORLD):
        assert _call(lib, _lib, name, st, _jit(_lib)) == 1
        assert b"a jitter struct with sample_type" in lib.rtxn_last_error() and name.encode() in lib.rtxn_last_error()


@pytest.mark.parametrize("name", ["rtxn_train_gradients_jitter", "rtxn_train_step_jitter"])
def test_one_call_forms_check_the_jitter_before_touching_a_device(name):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()

    def call(sample_type, vr, jitter):
        arg = _lib.TrainBatch() if name == "rtxn_train_gradients_jitter" else _lib.TrainStepArgs()
        b = arg if name == "rtxn_train_gradients_jitter" else arg.batch
        b.sample_type, b.vr_mode = sample_type, vr          # everything else NULL: an accepted jitter fails later, on the batch
        return getattr(lib, name)(C.byref(arg), None, C.byref(jitter) if jitter is not None else None, None)

    assert call(JITTER_WORLD, VR_NERF, None) == 1
    assert b"needs a jitter struct" in lib.rtxn_last_error() and name.encode() in lib.rtxn_last_error()
    assert call(MIDPOINT_WORLD, VR_NERF, _jit(_lib)) == 1
    assert b"a jitter struct with sample_type" in lib.rtxn_last_error() and name.encode() in lib.rtxn_last_error()
    assert call(JITTER_WORLD, VR_COMPAT, _jit(_lib)) == 1
    assert b"RTXN_VR_COMPAT" in lib.rtxn_last_error() and name.encode() in lib.rtxn_last_error()
    # accepted: the jitter rules pass and the call meets the batch's own checks; so does NULL + a deterministic type
    for st, j in ((JITTER_WORLD, _jit(_lib)), (MIDPOINT_WORLD, None)):
        assert call(st, VR_NERF, j) == 1
        assert b"NULL" in lib.rtxn_last_error() and b"jitter struct" not in lib.rtxn_last_error()
    assert getattr(lib, name)(None, None, None, None) == 1 and b"NULL" in lib.rtxn_last_error()


def test_plain_entries_keep_refusing_type_4():
    """The entry points without the struct have no seed to draw from: type 4 is RTXN_ERR_INVALID there, rtxn_sample included."""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    P = C.c_void_p(4096)
    assert lib.rtxn_sample(P, P, P, P, P, 4, 16, P, P, JITTER_WORLD, None) == 1
    assert b"rtxn_sample: unknown sample_type 4" in lib.rtxn_last_error()
    assert lib.rtxn_encode_frequency_segments(None, None, None, None, 4, JITTER_WORLD, 1.0, None, None, None) == 1
    assert b"rtxn_encode_frequency_segments:" in lib.rtxn_last_error() and b"needs a jitter struct" in lib.rtxn_last_error()
    assert lib.rtxn_hashgrid_backward_segments_live(None, None, None, 4, JITTER_WORLD, None, None, None, None, None) == 1
    assert b"rtxn_hashgrid_backward_segments_live:" in lib.rtxn_last_error() and b"needs a jitter struct" in lib.rtxn_last_error()


def test_trainer_refuses_jitter_in_compat_mode_before_allocating():
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match=re.escape("mode='nerf'")):
        Trainer(16, None, encoding="freq", device="cpu", mode="compat", sample_jitter=True)
