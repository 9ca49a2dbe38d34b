"""CPU-side checks of the training losses at the C-ABI boundary (rtxn_train_loss, rtxn_volrender_loss_train, rtxn_loss,
rtxn_train_gradients_loss, rtxn_train_step_loss): symbols and bindings, the struct's layout against the C
compiler, and the rules every entry point checks before any device is touched.  The Trainer's own refusals are checked here
too (they raise before allocating)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_volrender_loss_train", "rtxn_loss", "rtxn_train_gradients_loss", "rtxn_train_step_loss")
L2, L1, HUBER, REL = 0, 1, 2, 3
BG_NONE, BG_CONSTANT, BG_RANDOM = 0, 1, 2
VR_COMPAT, VR_NERF = 0, 1
P = C.c_void_p(4096)           # a fake device pointer: never launched from here


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_loss_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    assert lib.rtxn_version() == 100
    assert re.search(r"RTXN_LOSS_L2\s*=\s*0\s*,\s*RTXN_LOSS_L1\s*=\s*1\s*,\s*RTXN_LOSS_HUBER\s*=\s*2\s*,\s*RTXN_LOSS_RELATIVE_L2\s*=\s*3", _header())


def test_train_loss_layout_matches_the_header_and_the_c_compiler(tmp_path):
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index("typedef struct rtxn_train_loss {"):src.index("} rtxn_train_loss;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = [re.findall(r"([A-Za-z_]\w*)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    T = _lib.TrainLoss
    assert fields == [f[0] for f in T._fields_] == ["kind", "param", "opacity_weight", "opacity"]
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                 "sizeof(rtxn_train_loss), offsetof(rtxn_train_loss, kind), offsetof(rtxn_train_loss, param), "
                 "offsetof(rtxn_train_loss, opacity_weight), offsetof(rtxn_train_loss, opacity)); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(c), "-o", str(exe)])
    want = [C.sizeof(T), T.kind.offset, T.param.offset, T.opacity_weight.offset, T.opacity.offset]
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == want == [24, 0, 4, 8, 16]


def _loss(_lib, kind=HUBER, param=0.1, lam=0.0, opacity=None):
    s = _lib.TrainLoss()
    s.kind, s.param, s.opacity_weight, s.opacity = kind, param, lam, opacity
    return s


def _bg(_lib, mode, tc):
    b = _lib.TrainBackground()
    b.mode, b.target_channels, b.seed = mode, tc, 7
    b.color[:] = (1.0, 1.0, 1.0)
    return b


# (kind, param, lambda, background (mode, channels) or None, vr_mode) -> the field the message names
_REJECTED = [((7, 0.1, 0.0, None, VR_NERF), b"loss->kind"), ((-1, 0.1, 0.0, None, VR_NERF), b"loss->kind"),
             ((HUBER, 0.0, 0.0, None, VR_NERF), b"loss->param"), ((HUBER, -0.5, 0.0, None, VR_NERF), b"loss->param"),
             ((HUBER, float("nan"), 0.0, None, VR_NERF), b"loss->param"), ((HUBER, float("inf"), 0.0, None, VR_NERF), b"loss->param"),
             ((REL, 0.0, 0.0, None, VR_NERF), b"loss->param"), ((REL, -1e-2, 0.0, None, VR_NERF), b"loss->param"),
             ((REL, float("nan"), 0.0, None, VR_NERF), b"loss->param"),
             ((L1, 0.0, -0.1, None, VR_NERF), b"loss->opacity_weight"), ((L2, 0.0, -1.0, (BG_CONSTANT, 4), VR_NERF), b"loss->opacity_weight"),
             ((L2, 0.0, 0.5, None, VR_NERF), b"loss->opacity_weight"),                      # no RGBA targets
             ((HUBER, 0.1, 0.5, (BG_CONSTANT, 3), VR_NERF), b"loss->opacity_weight"),       # 3-channel targets
             ((HUBER, 0.1, 0.5, None, VR_COMPAT), b"RTXN_VR_COMPAT")]


@pytest.mark.parametrize("case,word", _REJECTED)
def test_loss_entries_reject_bad_specs_before_touching_a_device(case, word):
    """RTXN_ERR_INVALID (1) and a message naming the field, with or without a GPU; the buffers are never looked at."""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    kind, param, lam, bgc, vr = case
    spec = _loss(_lib, kind, param, lam)
    bg = _bg(_lib, *bgc) if bgc else None
    bgp = C.byref(bg) if bg is not None else None
    batch = _lib.TrainBatch()
    batch.vr_mode = vr                   # everything else NULL: an accepted spec would fail later, on the batch
    args = _lib.TrainStepArgs()
    args.batch.vr_mode = vr
    assert lib.rtxn_train_gradients_loss(C.byref(batch), bgp, None, C.byref(spec), None) == 1
    assert word in lib.rtxn_last_error() and b"rtxn_train_gradients_loss" in lib.rtxn_last_error()
    assert lib.rtxn_train_step_loss(C.byref(args), bgp, None, C.byref(spec), None) == 1
    assert word in lib.rtxn_last_error() and b"rtxn_train_step_loss" in lib.rtxn_last_error()
    if vr == VR_NERF:                    # the compositor has no mode argument: it is the NeRF one
        assert lib.rtxn_volrender_loss_train(P, P, P, P, 4, 32, P, 128.0, P, P, P, P, bgp, C.byref(spec), None) == 1
        assert word in lib.rtxn_last_error() and b"rtxn_volrender_loss_train" in lib.rtxn_last_error()
    if lam <= 0.0 and bgc is None and vr == VR_NERF:       # the stand-alone loss checks kind and param by the same rules
        assert lib.rtxn_loss(P, P, 12, C.byref(spec), 1.0, None, P, None, None) == 1
        assert word in lib.rtxn_last_error() and b"rtxn_loss" in lib.rtxn_last_error()


def test_stand_alone_loss_takes_no_alpha_term():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_loss(P, P, 12, C.byref(_loss(_lib, L1, 0.0, 0.5)), 1.0, None, P, None, None) == 1
    assert b"loss->opacity_weight" in lib.rtxn_last_error()
    assert lib.rtxn_loss(P, P, 12, C.byref(_loss(_lib, L1, 0.0, 0.0, P)), 1.0, None, P, None, None) == 1
    assert b"loss->opacity" in lib.rtxn_last_error()
    assert lib.rtxn_loss(P, P, -3, C.byref(_loss(_lib, L1)), 1.0, None, P, None, None) == 1 and b"n = -3" in lib.rtxn_last_error()


def test_valid_specs_reach_the_device_check_or_the_plain_checks():
    """A valid spec passes the loss rules: the compute entry points then need a device (RTXN_ERR_HIP = 2 without one; with one,
    an empty batch is RTXN_OK and touches no buffer), the batch entry points meet the batch's own checks."""
    import torch
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    want = 0 if torch.cuda.is_available() else 2
    rgba = _bg(_lib, BG_CONSTANT, 4)
    rand = _bg(_lib, BG_RANDOM, 4)
    for spec, bg in ((_loss(_lib, L1, 0.0), None), (_loss(_lib, HUBER, 0.1), None), (_loss(_lib, REL, 1e-2), None),
                     (_loss(_lib, HUBER, 0.1, 0.5, P), rgba), (_loss(_lib, L2, 0.0, 0.5), rand), (_loss(_lib, L2, 0.0, 0.0, P), None)):
        bgp = C.byref(bg) if bg is not None else None
        assert lib.rtxn_volrender_loss_train(P, P, P, P, 0, 32, P, 128.0, P, P, None, P, bgp, C.byref(spec), None) == want
        if want == 2:
            assert b"no HIP device" in lib.rtxn_last_error()
            assert lib.rtxn_volrender_loss_train(P, P, P, P, 4, 32, P, 128.0, P, P, P, P, bgp, C.byref(spec), None) == 2
        batch = _lib.TrainBatch()
        batch.vr_mode = VR_NERF
        assert lib.rtxn_train_gradients_loss(C.byref(batch), bgp, None, C.byref(spec), None) == 1
        assert b"NULL batch or model" in lib.rtxn_last_error()
    for spec in (_loss(_lib, L1, 0.0), _loss(_lib, HUBER, 0.1), _loss(_lib, REL, 1e-2)):
        assert lib.rtxn_loss(P, P, 0, C.byref(spec), 1.0, None, None, None, None) == want
    # NULL, or plain L2: the existing entry points' own checks, under their names
    for spec in (None, _loss(_lib, L2, 0.0)):
        sp = C.byref(spec) if spec is not None else None
        assert lib.rtxn_volrender_loss_train(P, P, P, P, -1, 32, P, 1.0, P, P, P, P, None, sp, None) == 1
        assert b"rtxn_volrender_l2_train: batch_size" in lib.rtxn_last_error()
        assert lib.rtxn_loss(P, P, -1, sp, 1.0, None, P, None, None) == 1 and b"rtxn_l2_loss" in lib.rtxn_last_error()
    assert lib.rtxn_volrender_loss_train(P, P, P, P, -1, 32, P, 1.0, P, P, P, P, None, C.byref(_loss(_lib, L1)), None) == 1
    assert b"rtxn_volrender_loss_train: batch_size" in lib.rtxn_last_error()
    assert lib.rtxn_train_gradients_loss(None, None, None, None, None) == 1 and b"NULL batch" in lib.rtxn_last_error()
    assert lib.rtxn_train_step_loss(None, None, None, None, None) == 1 and b"NULL arguments" in lib.rtxn_last_error()
    # a COMPAT batch takes the losses without an alpha term (rtxn_loss between the two compositor launches)
    batch = _lib.TrainBatch()
    batch.vr_mode = VR_COMPAT
    assert lib.rtxn_train_gradients_loss(C.byref(batch), None, None, C.byref(_loss(_lib, L1)), None) == 1
    assert b"NULL batch or model" in lib.rtxn_last_error()


def test_train_loss_struct_from_python():
    from rtx_nerf_amd import api
    s = api.train_loss()
    assert (s.kind, s.param, s.opacity_weight) == (api.LOSS_L2, 0.0, 0.0) and not s.opacity
    assert abs(api.train_loss("huber").param - 0.1) < 1e-8 and api.train_loss("huber").kind == api.LOSS_HUBER
    assert abs(api.train_loss("relative_l2").param - 1e-2) < 1e-9 and api.train_loss("relative_l2").kind == api.LOSS_RELATIVE_L2
    s = api.train_loss("l1", opacity_weight=0.25)
    assert (s.kind, s.opacity_weight) == (api.LOSS_L1, 0.25)
    assert api.train_loss("huber", param=0.5).param == 0.5
    with pytest.raises(ValueError):
        api.train_loss("smooth_l1")


@pytest.mark.parametrize("kw,word", [(dict(opacity_weight=0.1), "opacity_weight > 0"),
                                     (dict(opacity_weight=0.1, background=(1, 1, 1)), "opacity_weight > 0"),
                                     (dict(opacity_weight=-1.0), "opacity_weight = -1.0"),
                                     (dict(loss="mse"), "loss 'mse'"),
                                     (dict(loss="huber", loss_param=0.0), "loss_param"),
                                     (dict(loss="relative_l2", loss_param=float("nan")), "loss_param")])
def test_trainer_refuses_losses_it_cannot_train(kw, word):
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match=re.escape(word)):
        Trainer(16, None, encoding="freq", device="cpu", **kw)
