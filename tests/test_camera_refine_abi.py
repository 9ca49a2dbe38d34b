"""CPU-side checks of the intrinsics refinement's C surface (include/rtxn.h, rtxn_camera_refinement): the ctypes struct
against the header through gcc, every rule of rtxn_camera_refinement_check naming its field, and the rung rtxn_train_step_cameras
in the manner of tests/test_train_entry_names_abi.py.  No device is touched: every rule is checked before one is."""
import ctypes as C
import pathlib
import re
import subprocess

import pytest

import test_train_entry_names_abi as E

ROOT = pathlib.Path(__file__).resolve().parents[1]
P = E.P
FIELDS = ["model", "n_cameras", "width", "lr_focal", "lr_center", "lr_distortion", "max_log_focal", "max_center", "max_distortion", "beta1",
          "beta2", "eps", "params0", "params", "delta", "m", "v", "steps", "grad", "terms", "skip", "skipped", "drawn", "poses"]
# three ints and nine floats, then twelve pointers
WANT = [48 + 12 * 8] + [4 * i for i in range(12)] + [48 + 8 * i for i in range(12)]


def test_struct_matches_the_header(tmp_path):
    from rtx_nerf_amd import _lib
    name, T = "rtxn_camera_refinement", _lib.CameraRefinement
    src = (ROOT / "include" / "rtxn.h").read_text()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    declared = []
    for d in body.split(";"):
        if d.strip():
            declared += [re.findall(r"([A-Za-z_]\w*)\s*$", part.strip())[0] for part in d.split(",")]
    assert declared == [f[0] for f in T._fields_] == FIELDS
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("' + "%zu " * (len(FIELDS) + 1) + '\\n", '
                 f"sizeof({name}), " + ", ".join(f"offsetof({name}, {f})" for f in FIELDS) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(c), "-o", str(exe)])
    got = [C.sizeof(T)] + [getattr(T, f).offset for f in FIELDS]
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == got == WANT


_DEFAULTS = dict(model=1, n_cameras=2, width=16, lr_focal=2e-4, lr_center=1e-2, lr_distortion=1e-4, max_log_focal=0.25, max_center=8.0,
                 max_distortion=0.1, beta1=0.9, beta2=0.999, eps=1e-15)
_REJECTED = [(dict(lr_focal=-1e-4), b"lr_focal"), (dict(lr_center=-1.0), b"lr_center"), (dict(lr_distortion=-1e-9), b"lr_distortion"),
             (dict(lr_focal=float("nan")), b"lr_focal"), (dict(lr_center=float("inf")), b"lr_center"),
             (dict(beta1=1.0), b"beta1"), (dict(beta1=-0.1), b"beta1"), (dict(beta2=1.5), b"beta2"), (dict(beta2=float("nan")), b"beta2"),
             (dict(eps=0.0), b"eps"), (dict(eps=-1e-15), b"eps"),
             (dict(max_log_focal=-0.1), b"max_log_focal"), (dict(max_center=-1.0), b"max_center"), (dict(max_distortion=-1e-3), b"max_distortion"),
             (dict(max_center=float("nan")), b"max_center"),
             (dict(model=3), b"model"), (dict(model=-1), b"model"), (dict(n_cameras=0), b"n_cameras"), (dict(n_cameras=-2), b"n_cameras")]


def _struct(_lib, **kw):
    s = _lib.CameraRefinement()
    for k, v in {**_DEFAULTS, **kw}.items():
        setattr(s, k, v)
    return s


def test_the_check_accepts_the_defaults_frozen_groups_and_open_bounds():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    assert lib.rtxn_camera_refinement_check(C.byref(_struct(_lib))) == 0
    assert lib.rtxn_camera_refinement_check(C.byref(_struct(_lib, lr_focal=0.0, lr_center=0.0, lr_distortion=0.0))) == 0
    assert lib.rtxn_camera_refinement_check(C.byref(_struct(_lib, max_center=0.0, max_distortion=float("inf")))) == 0
    assert lib.rtxn_camera_refinement_check(None) == 1 and b"NULL" in lib.rtxn_last_error()
    s = api.camera_refinement("opencv_fisheye", 3, 40)                    # the configuration alone: no tensor, no device
    assert (s.model, s.n_cameras, s.width) == (2, 3, 40) and s.lr_focal == C.c_float(api.CAMERA_REFINE_DEFAULTS["lr_focal"]).value
    assert not s.params and not s.terms


@pytest.mark.parametrize("fields,word", _REJECTED, ids=[f"{list(f)[0]}={list(f.values())[0]}" for f, _ in _REJECTED])
def test_the_check_names_the_field(fields, word):
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    assert lib.rtxn_camera_refinement_check(C.byref(_struct(_lib, **fields))) == 1
    msg = lib.rtxn_last_error()
    assert msg.startswith(b"rtxn_camera_refinement_check: ") and b"cameras->" + word in msg, msg
    with pytest.raises(_lib.RtxnError, match=word.decode()):
        api.camera_refinement(**{**{k: v for k, v in _DEFAULTS.items()}, **fields})


def test_the_device_calls_refuse_missing_buffers_before_a_device_is_touched():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    s = _struct(_lib)
    for fn, args in (("rtxn_camera_gradients", (P, P, 4, P, C.byref(s), None)), ("rtxn_camera_step", (C.byref(s), None)),
                     ("rtxn_camera_compose", (C.byref(s), None))):
        assert getattr(lib, fn)(*args) == 1
        assert lib.rtxn_last_error().startswith(fn.encode() + b": cameras: NULL among params0"), lib.rtxn_last_error()
    for f in ("params0", "params", "delta", "m", "v", "steps", "grad"):
        setattr(s, f, P)
    assert lib.rtxn_camera_gradients(P, P, 4, P, C.byref(s), None) == 1 and b"cameras->terms" in lib.rtxn_last_error()
    s.terms = C.c_void_p(4096 + 8)
    assert lib.rtxn_camera_gradients(P, P, 4, P, C.byref(s), None) == 1 and b"16-byte" in lib.rtxn_last_error()
    s.terms = P
    assert lib.rtxn_camera_gradients(P, P, 0, P, C.byref(s), None) == 1 and b"n_rays = 0" in lib.rtxn_last_error()
    assert lib.rtxn_camera_gradients(P, None, 4, P, C.byref(s), None) == 1 and b"NULL among drawn" in lib.rtxn_last_error()
    s.width = 0
    assert lib.rtxn_camera_gradients(P, P, 4, P, C.byref(s), None) == 1 and b"cameras->width = 0" in lib.rtxn_last_error()


# ---- the rung rtxn_train_step_cameras ----------------------------------------------------------------------------------------
ACCEPTS = ("bg", "loss", "reg", "opt", "scaler", "ema", "rays", "pose", "cameras")


def _cameras(_lib, bad=False):
    s = _struct(_lib, lr_center=(-1.0 if bad else 1e-2))
    for f in ("params0", "params", "delta", "m", "v", "steps", "grad", "terms", "drawn", "poses"):
        setattr(s, f, P)
    return s, b"cameras->lr_center"


MAKE = dict(E.MAKE, cameras=_cameras)


def test_the_rung_called_with_nothing_reports_under_the_lowest_rung_it_amounts_to():
    from rtx_nerf_amd import _lib
    rc, msg = E._call(_lib, "step", "_cameras", ACCEPTS, [None], {})
    assert rc == 1 and msg == b"rtxn_train_step_reg: NULL arguments", msg


def test_the_rung_without_cameras_is_the_rays_rung():
    from rtx_nerf_amd import _lib
    structs = {name: MAKE[name](_lib, bad=(name == "pose"))[0] for name in ACCEPTS[:-1]}
    rc, msg = E._call(_lib, "step", "_cameras", ACCEPTS, [C.byref(E._step_args(_lib))], structs)
    assert rc == 1 and msg.startswith(b"rtxn_train_step_rays: ") and b"pose->lr" in msg, msg


@pytest.mark.parametrize("bad", ACCEPTS)
def test_the_rung_refuses_one_malformed_struct_under_its_own_name_and_names_the_field(bad):
    from rtx_nerf_amd import _lib
    structs, word = {}, None
    for name in ACCEPTS:
        structs[name], w = MAKE[name](_lib, bad=(name == bad))
        if name == bad:
            word = w
    rc, msg = E._call(_lib, "step", "_cameras", ACCEPTS, [C.byref(E._step_args(_lib))], structs)
    assert rc == 1 and msg.startswith(b"rtxn_train_step_cameras: ") and word in msg, msg


def test_the_rung_over_inactive_structs_reaches_the_plain_steps_own_checks():
    from rtx_nerf_amd import _lib
    structs = {"bg": E._bg(_lib)[0], "loss": E._loss(_lib)[0], "reg": E._reg(_lib)[0], "opt": E._opt(_lib, on=False)[0]}
    rc, msg = E._call(_lib, "step", "_cameras", ACCEPTS, [C.byref(E._step_args(_lib, mlp=False))], structs)
    assert rc == 1 and msg == b"rtxn_train_step: batch.mlp is NULL", msg


def test_cameras_without_rays_is_refused():
    from rtx_nerf_amd import _lib
    structs = {"cameras": _cameras(_lib)[0]}
    rc, msg = E._call(_lib, "step", "_cameras", ACCEPTS, [C.byref(E._step_args(_lib))], structs)
    assert rc == 1 and msg.startswith(b"rtxn_train_step_cameras: cameras without rays"), msg


def test_cameras_without_drawn_or_poses_is_refused():
    from rtx_nerf_amd import _lib
    for field in ("drawn", "poses"):
        structs = {"rays": E._rays(_lib)[0], "cameras": _cameras(_lib)[0]}
        setattr(structs["cameras"], field, None)
        rc, msg = E._call(_lib, "step", "_cameras", ACCEPTS, [C.byref(E._step_args(_lib))], structs)
        assert rc == 1 and msg.startswith(b"rtxn_train_step_cameras: cameras->drawn"), msg


def test_the_python_ladder_selects_the_rung():
    from rtx_nerf_amd import api
    opts = [None] * 10
    assert api._ladder_entry("rtxn_train_step", api._STEP_LADDER, opts) == ("rtxn_train_step", 0)
    opts[7] = object()
    assert api._ladder_entry("rtxn_train_step", api._STEP_LADDER, opts) == ("rtxn_train_step_rays", 9)
    opts[9] = object()
    assert api._ladder_entry("rtxn_train_step", api._STEP_LADDER, opts) == ("rtxn_train_step_cameras", 10)
