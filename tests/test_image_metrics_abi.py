"""CPU-side checks of the held-out evaluation at the C-ABI boundary (rtxn_image_metrics, rtxn_image_metrics_workspace_bytes,
rtxn_image_metrics_args): the symbols and their bindings, the struct's layout against the header, every validation rule before
any device is touched, and Trainer.evaluate's refusals (which raise before anything is allocated)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(4096)            # a non-NULL, 8-byte aligned pointer no rule ever follows
INVALID = 1


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def _header_fields(name):
    """field names of `typedef struct name { ... } name;` in header order (the method of test_abi.py)"""
    src = _header()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.split("{")[-1].strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?$", part.strip())[0])
    return fields


def test_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("rtxn_image_metrics", "rtxn_image_metrics_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert hasattr(lib, name), f"{name} not exported by librtxn.so"
    assert _lib.SYMBOLS["rtxn_image_metrics"] == (C.c_int, [C.POINTER(_lib.ImageMetricsArgs), C.c_void_p])
    assert _lib.SYMBOLS["rtxn_image_metrics_workspace_bytes"] == (C.c_size_t, [C.c_uint32, C.c_uint32])
    assert re.search(r"RTXN_METRICS_SSIM\s*=\s*1\b", code) and re.search(r"RTXN_METRICS_CLAMP\s*=\s*2\b", code)
    assert (api.METRICS_SSIM, api.METRICS_CLAMP) == (1, 2)
    assert callable(api.image_metrics) and callable(api.image_metrics_workspace)


def test_struct_layout_matches_the_header():
    from rtx_nerf_amd import _lib
    A = _lib.ImageMetricsArgs
    assert _header_fields("rtxn_image_metrics_args") == [f[0] for f in A._fields_] == [
        "set", "image", "pred", "background", "flags", "workspace", "workspace_bytes", "record"]
    # LP64: the 48-byte set, an int padded to 8, a pointer, three floats and an int, two pointers around a size_t
    assert C.sizeof(A) == 104
    assert [getattr(A, f).offset for f, _ in A._fields_] == [0, 48, 56, 64, 76, 80, 88, 96]


def test_layout_matches_the_c_compiler(tmp_path):
    """the same size and offsets from the header itself, through gcc"""
    import subprocess
    src = tmp_path / "sz.c"
    fields = ["image", "pred", "background", "flags", "workspace", "workspace_bytes", "record"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(fields) + ' %d %d\\n", sizeof(rtxn_image_metrics_args), '
                   + ", ".join(f"offsetof(rtxn_image_metrics_args, {f})" for f in fields)
                   + ", (int)RTXN_METRICS_SSIM, (int)RTXN_METRICS_CLAMP); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", f"-I{ROOT}/include", str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["104", "48", "56", "64", "76", "80", "88", "96", "1", "2"]


def _args(_lib, **kw):
    """arguments that pass every rule (fake pointers: never launched from here), then `kw` applied; set_* go to the image set"""
    a = _lib.ImageMetricsArgs()
    a.set.images, a.set.poses = P, None          # poses may be NULL: the kernels do not read them
    a.set.n_images, a.set.width, a.set.height, a.set.channels, a.set.format = 3, 16, 12, 3, 0
    a.set.focal_length, a.set.aspect_ratio = 2.0, 16 / 12
    a.image, a.pred, a.flags = 1, P, 3
    a.workspace, a.workspace_bytes, a.record = P, 16, P
    for k, v in kw.items():
        if k.startswith("set_"):
            setattr(a.set, k[4:], v)
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,needle", [
    (dict(set_images=None), b"NULL images or pred"), (dict(pred=None), b"NULL images or pred"),
    (dict(workspace=None), b"NULL workspace or record"), (dict(record=None), b"NULL workspace or record"),
    (dict(workspace=C.c_void_p(4100)), b"8-byte aligned"), (dict(record=C.c_void_p(4097)), b"8-byte aligned"),
    (dict(set_n_images=0), b"n_images = 0"), (dict(set_n_images=-2), b"n_images = -2"),
    (dict(image=-1), b"image = -1 outside [0, 3)"), (dict(image=3), b"image = 3 outside [0, 3)"),
    (dict(workspace_bytes=15), b"workspace_bytes = 15"), (dict(workspace_bytes=0), b"workspace_bytes = 0"),
    (dict(set_width=43, workspace_bytes=47), b"workspace_bytes = 47, 43 x 12 frames need 48"),
    (dict(set_width=0), b"width*height"), (dict(set_height=0), b"width*height"),
    (dict(set_width=4097, set_height=4096), b"width*height"), (dict(set_width=1 << 31, set_height=2), b"width*height"),
    (dict(set_channels=1), b"channels = 1"), (dict(set_channels=5), b"channels = 5"),
    (dict(set_format=2), b"image format 2"), (dict(set_format=-1), b"image format -1"),
    (dict(set_width=10), b"at least 11 x 11, not 10 x 12"), (dict(set_height=10, flags=1), b"at least 11 x 11, not 16 x 10"),
    (dict(flags=4), b"unknown flag bits in flags = 4"), (dict(flags=-1), b"unknown flag bits"),
])
def test_every_rule_is_checked_before_a_device_is_touched(kw, needle):
    """RTXN_ERR_INVALID (1) with a message that names the entry, with or without a GPU: no pointer is followed"""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_image_metrics(C.byref(_args(_lib, **kw)), None) == INVALID
    msg = lib.rtxn_last_error()
    assert msg.startswith(b"rtxn_image_metrics:") and needle in msg, msg


def test_null_args_small_frames_and_the_workspace_size():
    import torch
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_image_metrics(None, None) == INVALID and b"args is NULL" in lib.rtxn_last_error()
    # two doubles per 16 x 16 tile of windows, one tile for a frame too small to hold a window
    size = lib.rtxn_image_metrics_workspace_bytes
    assert [size(w, h) for w, h in ((5, 7), (11, 11), (26, 26), (27, 26), (37, 29), (64, 48), (800, 800), (4096, 4096))] == [
        16, 16, 16, 32, 64, 192, 16 * 50 * 50, 16 * 256 * 256]
    assert size(0, 5) == 0 and lib.rtxn_last_error().startswith(b"rtxn_image_metrics_workspace_bytes:")
    assert size(4097, 4096) == 0 and b"width*height" in lib.rtxn_last_error()
    if not torch.cuda.is_available():
        # without RTXN_METRICS_SSIM a 5 x 7 frame gets past the rules, and so does the largest frame with it: both fail on the
        # missing device, not on an argument
        assert lib.rtxn_image_metrics(C.byref(_args(_lib, set_width=5, set_height=7, flags=2)), None) == 2
        assert b"no HIP device" in lib.rtxn_last_error()
        big = _args(_lib, set_width=4096, set_height=4096, set_channels=4, set_format=1, workspace_bytes=16 * 256 * 256)
        assert lib.rtxn_image_metrics(C.byref(big), None) == 2 and b"no HIP device" in lib.rtxn_last_error()


def test_wrapper_checks_shapes_and_devices():
    import torch
    from rtx_nerf_amd import _lib, api
    s = api.ImageSet(torch.zeros((3, 12, 16, 3)), torch.zeros((3, 16)), 2.0)
    s4 = api.ImageSet(torch.zeros((3, 12, 16, 4)), torch.zeros((3, 16)), 2.0)
    assert api.image_metrics_workspace_bytes(16, 12) == 16
    rec, ws = torch.zeros(3, dtype=torch.float64), torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(_lib.RtxnError, match=r"pred of shape \(100, 3\)"):
        api.image_metrics(s, 0, torch.zeros((100, 3)), record=rec, workspace=ws)
    with pytest.raises(_lib.RtxnError, match=r"record of shape \(2,\)"):
        api.image_metrics(s, 0, torch.zeros((192, 3)), record=rec[:2], workspace=ws)
    with pytest.raises(_lib.RtxnError, match="4-channel image set needs background"):
        api.image_metrics(s4, 0, torch.zeros((192, 3)), record=rec, workspace=ws)
    with pytest.raises(_lib.RtxnError, match="CUDA tensor"):                        # host tensors never reach the library
        api.image_metrics(s, 0, torch.zeros((12, 16, 3)), record=rec, workspace=ws)


def _bare_trainer(**attrs):
    """evaluate()'s refusals need nothing of the trainer but these attributes, so none is built: without a GPU a Trainer cannot be"""
    from rtx_nerf_amd.train import Trainer
    tr = Trainer.__new__(Trainer)
    for k, v in attrs.items():
        setattr(tr, k, v)
    return tr


def test_evaluate_refuses_ema_of_a_trainer_without_it_before_allocating():
    import torch
    from rtx_nerf_amd import api
    tr = _bare_trainer(_ema=None, background=None)
    s = api.ImageSet(torch.zeros((3, 12, 16, 3)), torch.zeros((3, 16)), 2.0)
    with pytest.raises(RuntimeError, match=r"evaluate\(weights='ema'\): this trainer was made without ema_decay"):
        tr.evaluate(s, weights="ema")
    with pytest.raises(ValueError, match="weights = 'best'"):
        tr.evaluate(s, weights="best")
    assert "_eval_pipelines" not in tr.__dict__ and "_pipelines" not in tr.__dict__


@pytest.mark.parametrize("background", ["random", None])
def test_evaluate_refuses_an_rgba_set_without_a_colour_before_allocating(background):
    import torch
    from rtx_nerf_amd import api
    tr = _bare_trainer(_ema=None, background=background)
    s = api.ImageSet(torch.zeros((3, 12, 16, 4)), torch.zeros((3, 16)), 2.0)
    with pytest.raises(ValueError, match="a 4-channel image set needs a colour to composite its frames over"):
        tr.evaluate(s)
    with pytest.raises(ValueError, match="three floats"):
        tr.evaluate(s, background=(1.0, 1.0))
    with pytest.raises(ValueError, match=r"image 3 outside \[0, 3\)"):
        tr.evaluate(s, images=[0, 3], background=(1.0, 1.0, 1.0))
    assert "_eval_pipelines" not in tr.__dict__ and "_pipelines" not in tr.__dict__
