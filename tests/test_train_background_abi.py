"""CPU-side checks of training over a background at the C-ABI boundary (rtxn_train_background, rtxn_volrender_l2_train_ex,
rtxn_train_gradients_ex, rtxn_train_step_ex): symbols and bindings, the struct's field order, and the rules every _ex call
checks before any device is touched.  The Trainer's own refusals are checked here too (they raise before allocating)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_volrender_l2_train_ex", "rtxn_train_gradients_ex", "rtxn_train_step_ex")
BG_NONE, BG_CONSTANT, BG_RANDOM = 0, 1, 2
VR_COMPAT, VR_NERF = 0, 1


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_background_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    assert lib.rtxn_version() == 100


def test_train_background_matches_header_order():
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index("typedef struct rtxn_train_background {"):src.index("} rtxn_train_background;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = [re.findall(r"([A-Za-z_]\w*)\s*(?:\[\d+\])?\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.TrainBackground._fields_] == ["mode", "color", "seed", "step", "target_channels"]
    assert C.sizeof(_lib.TrainBackground) == 4 + 12 + 4 + 4 + 8 + 4 + 4      # step aligned to 8, struct padded to 8
    assert _lib.TrainBackground.step.offset == 24
    assert re.search(r"RTXN_BG_NONE\s*=\s*0\s*,\s*RTXN_BG_CONSTANT\s*=\s*1\s*,\s*RTXN_BG_RANDOM\s*=\s*2", src)
    assert re.search(r"RTXN_LOAD_RGBA\s*=\s*4\b", src)


def _bg(_lib, mode, tc, color=(1.0, 1.0, 1.0)):
    b = _lib.TrainBackground()
    b.mode, b.target_channels, b.seed = mode, tc, 7
    b.color[:] = color
    return b


# (mode, target_channels, vr_mode) -> a word of the message
_REJECTED = [((5, 3, VR_NERF), b"unknown background mode"), ((-1, 3, VR_NERF), b"unknown background mode"),
             ((BG_CONSTANT, 2, VR_NERF), b"target_channels"), ((BG_CONSTANT, 5, VR_NERF), b"target_channels"),
             ((BG_RANDOM, 3, VR_NERF), b"RANDOM"), ((BG_NONE, 4, VR_NERF), b"4-channel"),
             ((BG_CONSTANT, 3, VR_COMPAT), b"RTXN_VR_COMPAT"), ((BG_RANDOM, 4, VR_COMPAT), b"RTXN_VR_COMPAT"),
             ((BG_CONSTANT, 4, VR_COMPAT), b"RTXN_VR_COMPAT")]


@pytest.mark.parametrize("case,word", _REJECTED)
def test_ex_entries_reject_bad_backgrounds_before_touching_a_device(case, word):
    """RTXN_ERR_INVALID (1) and a message, with or without a GPU; the buffers are never looked at."""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    mode, tc, vr = case
    bg = _bg(_lib, mode, tc)
    P = C.c_void_p(4096)
    batch = _lib.TrainBatch()
    batch.vr_mode = vr                   # everything else NULL: an accepted background would fail later, on the batch
    args = _lib.TrainStepArgs()
    args.batch.vr_mode = vr
    assert lib.rtxn_train_gradients_ex(C.byref(batch), C.byref(bg), None) == 1
    assert word in lib.rtxn_last_error() and b"rtxn_train_gradients_ex" in lib.rtxn_last_error()
    assert lib.rtxn_train_step_ex(C.byref(args), C.byref(bg), None) == 1
    assert word in lib.rtxn_last_error() and b"rtxn_train_step_ex" in lib.rtxn_last_error()
    if vr == VR_NERF:                    # the compositor has no mode argument: it is the NeRF one
        assert lib.rtxn_volrender_l2_train_ex(P, P, P, P, 4, 32, P, 128.0, P, P, P, P, C.byref(bg), None) == 1
        assert word in lib.rtxn_last_error() and b"rtxn_volrender_l2_train_ex" in lib.rtxn_last_error()


def test_accepted_backgrounds_reach_the_plain_checks():
    """A valid background (or NULL / NONE with 3 channels) passes the background rules and meets the batch's own checks."""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    batch = _lib.TrainBatch()
    batch.vr_mode = VR_NERF
    for bg in (None, _bg(_lib, BG_NONE, 3), _bg(_lib, BG_CONSTANT, 3), _bg(_lib, BG_CONSTANT, 4), _bg(_lib, BG_RANDOM, 4)):
        assert lib.rtxn_train_gradients_ex(C.byref(batch), C.byref(bg) if bg is not None else None, None) == 1
        assert b"NULL batch or model" in lib.rtxn_last_error()
    assert lib.rtxn_train_gradients_ex(None, None, None) == 1 and b"NULL batch" in lib.rtxn_last_error()
    assert lib.rtxn_train_step_ex(None, None, None) == 1 and b"NULL arguments" in lib.rtxn_last_error()
    P = C.c_void_p(4096)
    bg = _bg(_lib, BG_CONSTANT, 4)
    assert lib.rtxn_volrender_l2_train_ex(P, P, P, P, -1, 32, P, 1.0, P, P, P, P, C.byref(bg), None) == 1
    assert b"batch_size" in lib.rtxn_last_error()


def test_train_background_struct_from_python():
    from rtx_nerf_amd import api
    b = api.train_background((0.25, 0.5, 1.0))
    assert b.mode == api.BG_CONSTANT and list(b.color) == [0.25, 0.5, 1.0] and b.target_channels == 3 and not b.step
    b = api.train_background("random", seed=-1, target_channels=4)
    assert b.mode == api.BG_RANDOM and b.seed == 0xFFFFFFFF and b.target_channels == 4
    assert api.train_background(None).mode == api.BG_NONE
    with pytest.raises(ValueError):
        api.train_background("white")
    with pytest.raises(ValueError):
        api.train_background((1.0, 1.0))


@pytest.mark.parametrize("kw,word", [(dict(mode="compat", background=(1, 1, 1)), "mode='nerf'"),
                                     (dict(background="random", target_channels=3), "needs 4"),
                                     (dict(target_channels=4), "RGBA needs a background"),
                                     (dict(background="black"), "'random'")])
def test_trainer_refuses_backgrounds_it_cannot_train(kw, word):
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match=re.escape(word)):
        Trainer(16, None, encoding="freq", device="cpu", **kw)


def test_trainer_refuses_a_background_with_the_three_launch_compositor(monkeypatch):
    from rtx_nerf_amd.train import Trainer
    monkeypatch.setenv("RTXN_TRAIN_FUSE_COMPOSITOR", "0")
    with pytest.raises(ValueError, match="RTXN_TRAIN_FUSE_COMPOSITOR=0"):
        Trainer(16, None, encoding="freq", device="cpu", background="random")
