"""CPU-side checks of the camera models at the C-ABI boundary (rtxn_camera_set and the five entry points of DESIGN 5.20): the
symbols and their bindings, the struct's layout against the header and the C compiler, every argument rule before any device is
touched, the host's invertibility check, and loader.read_cameras on files written here."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(4096)            # a non-NULL pointer no rule ever follows
INVALID = 1
NEW = ("rtxn_camera_set_check", "rtxn_camera_rays", "rtxn_draw_batch_cameras", "rtxn_render_frame_rays", "rtxn_render_count_segments_rays")


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_the_five_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported by librtxn.so"
        assert name in _lib.SYMBOLS
    u32, p = C.c_uint32, C.c_void_p
    cs = C.POINTER(_lib.CameraSet)
    assert _lib.SYMBOLS["rtxn_camera_set_check"] == (C.c_int, [cs, C.c_int])
    assert _lib.SYMBOLS["rtxn_camera_rays"] == (C.c_int, [cs, C.c_int, p, u32, u32, u32, u32, p, p, p])
    assert _lib.SYMBOLS["rtxn_draw_batch_cameras"] == (C.c_int, [C.POINTER(_lib.DrawBatchArgs), cs, p])
    assert _lib.SYMBOLS["rtxn_render_frame_rays"] == (C.c_int, [p, C.c_int, p, p, u32, u32, C.POINTER(_lib.RenderOutputs), p])
    assert _lib.SYMBOLS["rtxn_render_count_segments_rays"] == (C.c_int, [p, p, p, u32, u32, C.POINTER(C.c_long), p])
    for k, v in (("PINHOLE", 0), ("OPENCV", 1), ("OPENCV_FISHEYE", 2)):
        assert re.search(rf"RTXN_CAMERA_{k}\s*=\s*{v}\b", code) and getattr(api, f"CAMERA_{k}") == v
    assert re.search(r"RTXN_CAMERA_PARAMS\s*=\s*12\b", code) and api.CAMERA_PARAMS == 12
    assert re.search(r"#define RTXN_VERSION 100\b", code) and lib.rtxn_version() == 100


def test_struct_layout_matches_the_header_and_the_c_compiler(tmp_path):
    from rtx_nerf_amd import _lib
    src = _header()
    body = re.sub(r"/\*.*?\*/", "", src[src.index("typedef struct rtxn_camera_set {"):src.index("} rtxn_camera_set;")], flags=re.S)
    fields = [re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", d.split("{")[-1].strip())[0] for d in body.split(";") if d.split("{")[-1].strip()]
    S = _lib.CameraSet
    assert fields == [f[0] for f in S._fields_] == ["model", "n_cameras", "params"]
    assert C.sizeof(S) == 16 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8]
    csrc = tmp_path / "sz.c"
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                    "sizeof(rtxn_camera_set), offsetof(rtxn_camera_set, model), offsetof(rtxn_camera_set, n_cameras), "
                    "offsetof(rtxn_camera_set, params), sizeof(rtxn_image_set), sizeof(rtxn_draw_batch_args)); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(csrc), "-o", str(exe)])
    # the two structs the camera entries take beside it keep their layouts
    assert subprocess.check_output([str(exe)], text=True).split() == ["16", "0", "4", "8", "48", "96"]


def _cams(_lib, model=1, n=3, params=P):
    s = _lib.CameraSet()
    s.model, s.n_cameras, s.params = model, n, params
    return s


def _draw(_lib, **kw):
    a = _lib.DrawBatchArgs()
    a.set.images, a.set.poses = P, P
    a.set.n_images, a.set.width, a.set.height, a.set.channels, a.set.format = 3, 16, 12, 3, 0
    a.n_rays, a.seed = 256, 7
    a.rays_o, a.rays_d, a.targets = P, P, P
    for k, v in kw.items():
        if k.startswith("set_"):
            setattr(a.set, k[4:], v)
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,n_images,needle", [
    (dict(model=3), 3, b"unknown camera model 3"), (dict(model=-1), 3, b"unknown camera model -1"),
    (dict(n=2), 3, b"n_cameras = 2 must be 1 or n_images = 3"), (dict(n=0), 3, b"n_cameras = 0"), (dict(n=4), 3, b"n_cameras = 4"),
    (dict(params=None), 3, b"NULL camera params"), (dict(), 0, b"n_images = 0"),
])
def test_camera_set_check_rules(kw, n_images, needle):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_camera_set_check(C.byref(_cams(_lib, **kw)), n_images) == INVALID
    msg = lib.rtxn_last_error()
    assert msg.startswith(b"rtxn_camera_set_check:") and needle in msg, msg


def test_camera_set_check_accepts_one_or_n_cameras_of_every_model():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_camera_set_check(None, 3) == INVALID and b"cameras is NULL" in lib.rtxn_last_error()
    for model in (0, 1, 2):
        for n in (1, 3):
            assert lib.rtxn_camera_set_check(C.byref(_cams(_lib, model=model, n=n)), 3) == 0


@pytest.mark.parametrize("cams,args,needle", [
    (None, {}, b"cameras is NULL"), (dict(model=7), {}, b"unknown camera model 7"), (dict(params=None), {}, b"NULL camera params"),
    (dict(n=0), {}, b"n_cameras = 0 must be >= 1"),
    (dict(), dict(camera=3), b"camera = 3 out of [0,3)"), (dict(), dict(camera=-1), b"camera = -1 out of"),
    (dict(), dict(look_at=None), b"NULL look_at"), (dict(), dict(rays_o=None), b"NULL look_at"), (dict(), dict(rays_d=None), b"NULL look_at"),
    (dict(), dict(width=0), b"width*height"), (dict(), dict(height=0), b"width*height"), (dict(), dict(width=1 << 16, height=1 << 15), b"width*height"),
    (dict(), dict(ray_begin=1200), b"ray window [1200,+1)"), (dict(), dict(ray_begin=1000, ray_count=201), b"ray window [1000,+201)"),
    (dict(), dict(ray_begin=0xFFFFFFFF, ray_count=2), b"ray window"),
])
def test_camera_rays_rules_are_checked_before_a_device_is_touched(cams, args, needle):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    a = dict(camera=0, look_at=P, width=40, height=30, ray_begin=0, ray_count=1, rays_o=P, rays_d=P)
    a.update(args)
    s = None if cams is None else C.byref(_cams(_lib, **cams))
    assert lib.rtxn_camera_rays(s, a["camera"], a["look_at"], a["width"], a["height"], a["ray_begin"], a["ray_count"], a["rays_o"],
                                a["rays_d"], None) == INVALID
    msg = lib.rtxn_last_error()
    assert msg.startswith(b"rtxn_camera_rays:") and needle in msg, msg


@pytest.mark.parametrize("kw,needle", [
    (dict(set_images=None), b"NULL images or poses"), (dict(set_poses=None), b"NULL images or poses"),
    (dict(rays_o=None), b"NULL rays_o"), (dict(rays_d=None), b"NULL rays_o"), (dict(targets=None), b"NULL rays_o"),
    (dict(set_n_images=0), b"n_images = 0"), (dict(n_rays=0), b"n_rays = 0"), (dict(n_rays=-1), b"n_rays = -1"),
    (dict(set_width=0), b"width*height"), (dict(set_width=4097, set_height=4096), b"width*height"),
    (dict(set_channels=2), b"channels = 2"), (dict(set_format=2), b"image format 2"),
])
def test_draw_batch_cameras_applies_the_rules_of_draw_batch(kw, needle):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_draw_batch_cameras(C.byref(_draw(_lib, **kw)), C.byref(_cams(_lib)), None) == INVALID
    msg = lib.rtxn_last_error()
    assert msg.startswith(b"rtxn_draw_batch_cameras:") and needle in msg, msg


@pytest.mark.parametrize("cams,needle", [
    (None, b"cameras is NULL"), (dict(model=3), b"unknown camera model 3"), (dict(n=2), b"n_cameras = 2 must be 1 or n_images = 3"),
    (dict(params=None), b"NULL camera params"),
])
def test_draw_batch_cameras_applies_the_rules_of_the_camera_set(cams, needle):
    import torch
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    s = None if cams is None else C.byref(_cams(_lib, **cams))
    assert lib.rtxn_draw_batch_cameras(C.byref(_draw(_lib)), s, None) == INVALID
    msg = lib.rtxn_last_error()
    assert msg.startswith(b"rtxn_draw_batch_cameras:") and needle in msg, msg
    assert lib.rtxn_draw_batch_cameras(None, C.byref(_cams(_lib)), None) == INVALID and b"args is NULL" in lib.rtxn_last_error()
    if not torch.cuda.is_available():      # valid arguments get past every rule and fail on the missing device
        assert lib.rtxn_draw_batch_cameras(C.byref(_draw(_lib)), C.byref(_cams(_lib, n=1)), None) == 2
        assert b"no HIP device" in lib.rtxn_last_error()


def test_frame_entries_over_rays_refuse_null_arguments():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    o = _lib.RenderOutputs()
    n = C.c_long(0)
    for r, ro, rd in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.rtxn_render_frame_rays(r, 0, ro, rd, 0, 0, C.byref(o), None) == INVALID
        assert lib.rtxn_last_error().startswith(b"rtxn_render_frame_rays: NULL argument")
        assert lib.rtxn_render_count_segments_rays(r, ro, rd, 0, 0, C.byref(n), None) == INVALID
        assert lib.rtxn_last_error().startswith(b"rtxn_render_count_segments_rays: NULL argument")
    assert lib.rtxn_render_count_segments_rays(P, P, P, 0, 0, None, None) == INVALID


# --------------------------------------------------------------------------- the Python holders (host tensors: no device needed)
def test_camera_params_and_camera_set():
    import torch
    from rtx_nerf_amd import api
    row = api.camera_params(32, 30, 18.3, 16.1, k1=-0.3, k2=0.1, k3=-0.01, p1=0.001, p2=-0.001)
    assert row == [32.0, 30.0, 18.3, 16.1, -0.3, 0.1, -0.01, 0.0, 0.001, -0.001, 0.0, 0.0]
    cs = api.camera_set("opencv", row, width=40, height=30, device="cpu")
    assert (cs.model, cs.n_cameras) == (api.CAMERA_OPENCV, 1) and cs.params.shape == (1, 12) and cs.params.dtype == torch.float32
    cs3 = api.camera_set("opencv_fisheye", [api.camera_params(32, 30, 18.3, 16.1, k1=-0.1, k2=0.01)] * 3, width=40, height=30, device="cpu")
    assert (cs3.model, cs3.n_cameras) == (api.CAMERA_OPENCV_FISHEYE, 3)
    s = api.ImageSet(torch.zeros((3, 30, 40, 3)), torch.zeros((3, 16)), cameras=cs3)
    assert s.cameras is cs3 and s.focal_length is None and s.camera_of(2) == 2
    assert api.ImageSet(torch.zeros((3, 30, 40, 3)), torch.zeros((3, 16)), 2.0, cameras=cs).camera_of(2) == 0
    with pytest.raises(ValueError, match="focal_length is required without cameras"):
        api.ImageSet(torch.zeros((3, 30, 40, 3)), torch.zeros((3, 16)))
    with pytest.raises(ValueError, match="a CameraSet of 1 or 2 cameras"):
        api.ImageSet(torch.zeros((2, 30, 40, 3)), torch.zeros((2, 16)), cameras=cs3)
    with pytest.raises(ValueError, match="model 'fisheye'"):
        api.camera_set("fisheye", row, device="cpu")
    with pytest.raises(ValueError, match=r"params of shape \(1, 11\)"):
        api.camera_set("pinhole", row[:11], device="cpu")
    with pytest.raises(ValueError, match="camera 0: fx = 0.0"):
        api.camera_set("pinhole", api.camera_params(0, 19, 18, 16), device="cpu")


@pytest.mark.parametrize("with_size", [True, False])
def test_camera_set_refuses_parameters_that_are_not_invertible(with_size):
    """k1 = -2: x (1 - 2 r^2) turns back at r = 0.41, so most of the frame has no pre-image; the error names camera and pixel"""
    from rtx_nerf_amd import api
    good = api.camera_params(32, 30, 18.3, 16.1, k1=-0.05)
    bad = api.camera_params(32, 30, 18.3, 16.1, k1=-2.0)
    kw = dict(width=40, height=30) if with_size else {}
    api.camera_set("opencv", [good, good], device="cpu", **kw)
    with pytest.raises(ValueError, match=r"camera 1 \(opencv\) is not invertible .* at pixel \(\d+\.\d+, \d+\.\d+\)"):
        api.camera_set("opencv", [good, bad], device="cpu", **kw)
    with pytest.raises(ValueError, match=r"camera 0 \(opencv_fisheye\) is not invertible"):
        api.camera_set("opencv_fisheye", api.camera_params(32, 30, 18.3, 16.1, k1=-2.0), device="cpu", **kw)
    api.camera_set("pinhole", bad, device="cpu", **kw)          # the pinhole reads no coefficient


def test_every_coefficient_set_of_the_gpu_tests_passes_the_host_check():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _camera_float64 as R
    from rtx_nerf_amd import api
    for name, model, row in R.all_cases():
        api.camera_set([k for k, v in api.CAMERA_MODELS.items() if v == model][0], row, width=R.W, height=R.H, device="cpu")


# --------------------------------------------------------------------------- loader.read_cameras
def _write(tmp_path, doc):
    p = tmp_path / "transforms.json"
    p.write_text(json.dumps(doc))
    return str(p)


def test_read_cameras_global_keys(tmp_path):
    from rtx_nerf_amd import loader
    doc = dict(camera_model="OPENCV", fl_x=1111.0, fl_y=1113.5, cx=640.25, cy=359.5, k1=-0.1, k2=0.02, k3=0.001, p1=1e-3, p2=-2e-3, w=1280, h=720,
               frames=[dict(file_path="a"), dict(file_path="b")])
    model, P_ = loader.read_cameras(_write(tmp_path, doc), 1280, 720)
    assert model == "opencv" and P_.shape == (1, 12) and P_.dtype == np.float32
    np.testing.assert_array_equal(P_[0], np.float32([1111.0, 1113.5, 640.25, 359.5, -0.1, 0.02, 0.001, 0.0, 1e-3, -2e-3, 0, 0]))


def test_read_cameras_per_frame_keys_and_the_rescale(tmp_path):
    from rtx_nerf_amd import loader
    doc = dict(camera_model="OPENCV_FISHEYE", w=800, h=600, k1=0.05, k2=-0.01, k3=0.002, k4=-0.0003,
               frames=[dict(fl_x=400.0, fl_y=410.0, cx=401.0, cy=299.0), dict(fl_x=420.0, cx=380.0, cy=310.0, k1=0.04),
                       dict(fl_x=400.0, fl_y=400.0, w=1600, h=1200, cx=800.0, cy=600.0)])
    model, P_ = loader.read_cameras(_write(tmp_path, doc), 400, 300)       # loaded at half size
    assert model == "opencv_fisheye" and P_.shape == (3, 12)
    np.testing.assert_array_equal(P_[0], np.float32([200.0, 205.0, 200.5, 149.5, 0.05, -0.01, 0.002, -0.0003, 0, 0, 0, 0]))
    np.testing.assert_array_equal(P_[1], np.float32([210.0, 210.0, 190.0, 155.0, 0.04, -0.01, 0.002, -0.0003, 0, 0, 0, 0]))
    np.testing.assert_array_equal(P_[2, :4], np.float32([100.0, 100.0, 200.0, 150.0]))         # its own w, h: a quarter
    # anisotropic: x by 2, y by 0.5
    _, Q = loader.read_cameras(_write(tmp_path, dict(fl_x=100.0, fl_y=120.0, cx=50.0, cy=40.0, w=100, h=80, frames=[{}])), 200, 40)
    np.testing.assert_array_equal(Q[0, :4], np.float32([200.0, 60.0, 100.0, 20.0]))


def test_read_cameras_model_rules_and_the_fallback(tmp_path):
    import math
    from rtx_nerf_amd import loader
    # no camera_model: pinhole without coefficients, opencv with one, fisheye with instant-ngp's flag
    assert loader.read_cameras(_write(tmp_path, dict(fl_x=50.0, frames=[])), 64, 48)[0] == "pinhole"
    assert loader.read_cameras(_write(tmp_path, dict(fl_x=50.0, k1=0.01, frames=[])), 64, 48)[0] == "opencv"
    assert loader.read_cameras(_write(tmp_path, dict(fl_x=50.0, is_fisheye=True, k1=0.01, frames=[])), 64, 48)[0] == "opencv_fisheye"
    # defaults: fl_y = fl_x, the principal point at the centre
    np.testing.assert_array_equal(loader.read_cameras(_write(tmp_path, dict(fl_x=50.0, frames=[])), 64, 48)[1][0, :4], np.float32([50, 50, 32, 24]))
    # camera_angle_x: a centred pinhole over the loaded size
    model, P_ = loader.read_cameras(_write(tmp_path, dict(camera_angle_x=0.6911112070083618, frames=[dict(file_path="r_0")])), 800, 800)
    assert model == "pinhole" and P_.shape == (1, 12)
    f = np.float32(400.0 / math.tan(0.5 * 0.6911112070083618))
    np.testing.assert_array_equal(P_[0], np.float32([f, f, 400, 400] + [0] * 8))
    with pytest.raises(ValueError, match="neither fl_x nor camera_angle_x"):
        loader.read_cameras(_write(tmp_path, dict(frames=[])), 8, 8)
    with pytest.raises(ValueError, match="camera_model 'EQUIRECTANGULAR'"):
        loader.read_cameras(_write(tmp_path, dict(fl_x=5.0, camera_model="EQUIRECTANGULAR", frames=[])), 8, 8)
    with pytest.raises(ValueError, match="different camera models"):
        loader.read_cameras(_write(tmp_path, dict(fl_x=5.0, frames=[dict(camera_model="OPENCV"), dict(camera_model="OPENCV_FISHEYE")])), 8, 8)


def test_read_cameras_feeds_camera_set(tmp_path):
    from rtx_nerf_amd import api, loader
    doc = dict(camera_model="OPENCV", fl_x=32.0, fl_y=30.0, cx=18.3, cy=16.1, k1=-0.3, k2=0.1, k3=-0.01, p1=0.001, p2=-0.001, w=40, h=30, frames=[{}])
    model, P_ = loader.read_cameras(_write(tmp_path, doc), 40, 30)
    cs = api.camera_set(model, P_, width=40, height=30, device="cpu")
    assert cs.n_cameras == 1 and cs.model == api.CAMERA_OPENCV
