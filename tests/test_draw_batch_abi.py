"""CPU-side checks of the device batch draw at the C-ABI boundary (rtxn_draw_batch, rtxn_image_set, rtxn_draw_batch_args): the
symbol and its binding, the two structs' layouts against the header, every validation rule before any device is touched, and the
Trainer's channel rules (which raise before anything is allocated)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(4096)            # a non-NULL pointer no rule ever follows
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
            fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())[0])
    return fields


def test_draw_batch_is_declared_exported_and_bound():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    assert re.search(r"\brtxn_draw_batch\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    assert hasattr(lib, "rtxn_draw_batch"), "rtxn_draw_batch not exported by librtxn.so"
    assert _lib.SYMBOLS["rtxn_draw_batch"] == (C.c_int, [C.POINTER(_lib.DrawBatchArgs), C.c_void_p])
    assert re.search(r"RTXN_IMAGE_F32\s*=\s*0\b", _header()) and re.search(r"RTXN_IMAGE_U8\s*=\s*1\b", _header())
    assert (api.IMAGE_F32, api.IMAGE_U8) == (0, 1)


def test_struct_layouts_match_the_header():
    from rtx_nerf_amd import _lib
    assert _header_fields("rtxn_image_set") == [f[0] for f in _lib.ImageSet._fields_] == [
        "images", "poses", "n_images", "width", "height", "channels", "format", "focal_length", "aspect_ratio"]
    assert _header_fields("rtxn_draw_batch_args") == [f[0] for f in _lib.DrawBatchArgs._fields_] == [
        "set", "n_rays", "seed", "step", "rays_o", "rays_d", "targets", "drawn"]
    # LP64: two pointers, seven 4-byte scalars, padded to 8; then two ints and five pointers
    assert C.sizeof(_lib.ImageSet) == 48 and C.sizeof(_lib.DrawBatchArgs) == 96
    S, A = _lib.ImageSet, _lib.DrawBatchArgs
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 20, 24, 28, 32, 36, 40]
    assert [getattr(A, f).offset for f, _ in A._fields_] == [0, 48, 52, 56, 64, 72, 80, 88]


def test_layouts_match_the_c_compiler(tmp_path):
    """the same sizes and offsets from the header itself, through gcc"""
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(rtxn_image_set), sizeof(rtxn_draw_batch_args), offsetof(rtxn_image_set, aspect_ratio), "
                   "offsetof(rtxn_draw_batch_args, n_rays), offsetof(rtxn_draw_batch_args, step), offsetof(rtxn_draw_batch_args, drawn)); "
                   "return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", f"-I{ROOT}/include", str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["48", "96", "40", "48", "56", "88"]


def _args(_lib, **kw):
    """arguments that pass every rule (fake pointers: never launched from here), then `kw` applied; set_* go to the image set"""
    a = _lib.DrawBatchArgs()
    a.set.images, a.set.poses = P, P
    a.set.n_images, a.set.width, a.set.height, a.set.channels, a.set.format = 3, 16, 12, 3, 0
    a.set.focal_length, a.set.aspect_ratio = 2.0, 16 / 12
    a.n_rays, a.seed = 256, 7
    a.rays_o, a.rays_d, a.targets = P, P, P
    for k, v in kw.items():
        if k.startswith("set_"):
            setattr(a.set, k[4:], v)
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,needle", [
    (dict(set_images=None), b"NULL images or poses"), (dict(set_poses=None), b"NULL images or poses"),
    (dict(rays_o=None), b"NULL rays_o"), (dict(rays_d=None), b"NULL rays_o"), (dict(targets=None), b"NULL rays_o"),
    (dict(set_n_images=0), b"n_images = 0"), (dict(set_n_images=-2), b"n_images = -2"),
    (dict(n_rays=0), b"n_rays = 0"), (dict(n_rays=-1), b"n_rays = -1"),
    (dict(set_width=0), b"width*height"), (dict(set_height=0), b"width*height"),
    (dict(set_width=4097, set_height=4096), b"width*height"), (dict(set_width=1 << 31, set_height=2), b"width*height"),
    (dict(set_channels=1), b"channels = 1"), (dict(set_channels=5), b"channels = 5"),
    (dict(set_format=2), b"image format 2"), (dict(set_format=-1), b"image format -1"),
])
def test_every_rule_is_checked_before_a_device_is_touched(kw, needle):
    """RTXN_ERR_INVALID (1) with a message that names the entry, with or without a GPU: no pointer is followed"""
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_draw_batch(C.byref(_args(_lib, **kw)), None) == INVALID
    msg = lib.rtxn_last_error()
    assert msg.startswith(b"rtxn_draw_batch:") and needle in msg, msg


def test_null_args_and_the_largest_frame():
    import torch
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_draw_batch(None, None) == INVALID and b"args is NULL" in lib.rtxn_last_error()
    if not torch.cuda.is_available():
        # 4096 x 4096 = 1 << 24 pixels is allowed: the call gets past its rules and fails on the missing device, not on an argument
        assert lib.rtxn_draw_batch(C.byref(_args(_lib, set_width=4096, set_height=4096, set_channels=4, set_format=1)), None) == 2
        assert b"no HIP device" in lib.rtxn_last_error()


def test_wrapper_checks_shapes_and_devices():
    import torch
    from rtx_nerf_amd import _lib, api
    img = torch.zeros((3, 12, 16, 3))
    poses = torch.zeros((3, 4, 4))
    s = api.ImageSet(img, poses, 2.0)
    assert (s.n_images, s.height, s.width, s.channels, s.format) == (3, 12, 16, 3, api.IMAGE_F32) and s.aspect_ratio == 16 / 12
    assert s.poses.shape == (3, 16) and s.nbytes() == 3 * 12 * 16 * 3 * 4 + 3 * 64
    assert api.ImageSet(img.to(torch.uint8), poses.reshape(3, 16), 2.0, aspect_ratio=1.0).format == api.IMAGE_U8
    for bad_img, bad_poses in ((img[0], poses), (torch.zeros((3, 12, 16, 2)), poses), (img.double(), poses), (img, poses[:2]),
                               (img, poses.double()), (img, torch.zeros((3, 8, 2)))):
        with pytest.raises(ValueError, match="ImageSet"):
            api.ImageSet(bad_img, bad_poses, 2.0)
    o = torch.zeros((8, 3))
    with pytest.raises(_lib.RtxnError, match=r"targets of shape \(8, 3\)"):      # a 4-channel set needs [n, 4] targets
        api.draw_batch(api.ImageSet(torch.zeros((3, 12, 16, 4)), poses, 2.0), 8, 0, None, o, o, o)
    with pytest.raises(_lib.RtxnError, match="rays_o of shape"):
        api.draw_batch(s, 9, 0, None, o, o, o)
    with pytest.raises(_lib.RtxnError, match="CUDA tensor"):                        # host tensors never reach the library
        api.draw_batch(s, 8, 0, None, o, o, o)


@pytest.mark.parametrize("set_channels,target_channels", [(4, 3), (3, 4)])
def test_trainer_refuses_a_set_of_the_wrong_width_before_allocating(set_channels, target_channels):
    """attach_images looks at the channel counts first: a 4-channel set needs a trainer with RGBA targets, a trainer with RGBA
    targets needs a 4-channel set.  (The check needs nothing of the trainer but its target width, so none is built here: without a
    GPU a Trainer cannot be.)"""
    import torch
    from rtx_nerf_amd import api
    from rtx_nerf_amd.train import Trainer
    tr = Trainer.__new__(Trainer)
    tr.target_channels, tr.image_set = target_channels, None
    s = api.ImageSet(torch.zeros((3, 12, 16, set_channels)), torch.zeros((3, 16)), 2.0)
    with pytest.raises(ValueError, match=f"a {set_channels}-channel image set for a trainer that takes {target_channels}-channel"):
        tr.attach_images(s)
    assert tr.image_set is None and not hasattr(tr, "draw_rays_o")
    for fn, kw in ((Trainer.step_images, {}), (Trainer.capture_step, dict(n_rays=8, draw=True)), (Trainer.entry_args, dict(n_rays=8, draw=True))):
        with pytest.raises(RuntimeError, match="attach_images"):
            fn(tr, **kw)


@pytest.mark.parametrize("holder", ["graph", "entry"])
def test_trainer_refuses_another_set_once_a_graph_or_an_entry_struct_draws(holder):
    """a graph captured with draw=True and the struct of entry_args(draw=True) hold the attached set's addresses: attaching
    another set behind them is refused, before anything of the trainer changes"""
    import torch
    from rtx_nerf_amd import api
    from rtx_nerf_amd.train import Trainer
    tr = Trainer.__new__(Trainer)
    tr.target_channels, tr.image_set = 3, "the first set"
    if holder == "graph":
        tr._g_draw = True
    else:
        tr._entry_draw = object()
    s = api.ImageSet(torch.zeros((3, 12, 16, 3)), torch.zeros((3, 16)), 2.0)
    with pytest.raises(RuntimeError, match="attach_images: a captured graph or an entry struct"):
        tr.attach_images(s)
    assert tr.image_set == "the first set"
