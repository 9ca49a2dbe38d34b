"""CPU-side checks of the ray gradients and the pose refinement at the C-ABI boundary (rtxn_ray_gradients, rtxn_pose_refinement and
the entry points that take them): symbols and bindings, the structs' layout against the C compiler, every rule
refused with its field named before any device is touched (on fake device pointers), and the Trainer's ValueErrors, raised
before anything is allocated."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_ray_gradients_supported", "rtxn_hashgrid_input_gradient_segments", "rtxn_ray_gradients_reduce",
               "rtxn_pose_refinement_check", "rtxn_pose_gradients", "rtxn_pose_step", "rtxn_pose_compose", "rtxn_train_gradients_rays",
               "rtxn_train_step_rays")
P = C.c_void_p(4096)           # a fake device pointer: never launched from here
RAY_FIELDS = ["t_start", "t_end", "dstart", "dend", "d_origin", "d_direction"]
POSE_FIELDS = ["n_images", "poses0", "poses", "delta", "m", "v", "steps", "grad", "lr", "beta1", "beta2", "eps", "skip", "skipped", "drawn"]


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    for n in ("ray_gradients", "pose_refinement", "hashgrid_input_gradient_segments", "ray_gradients_reduce", "pose_gradients", "pose_step",
              "pose_compose", "ray_gradients_supported"):
        assert callable(getattr(api, n))
    assert callable(api.HashGrid.input_gradient_segments)
    sig = inspect.signature(api.train_step).parameters
    assert sig["rays"].default is None and sig["pose"].default is None
    assert inspect.signature(api.train_gradients).parameters["rays"].default is None
    from rtx_nerf_amd.train import Trainer
    assert inspect.signature(Trainer.__init__).parameters["ray_gradients"].default is False
    assert inspect.signature(Trainer.attach_images).parameters["refine_poses"].default is None
    for n in ("refined_poses", "reset_poses"):
        assert callable(getattr(Trainer, n))
    assert lib.rtxn_version() == 100


@pytest.mark.parametrize("name,T,fields,want", [
    ("rtxn_ray_gradients", "RayGradients", RAY_FIELDS, [48, 0, 8, 16, 24, 32, 40]),
    ("rtxn_pose_refinement", "PoseRefinement", POSE_FIELDS, [104, 0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 80, 88, 96])])
def test_struct_layouts_match_the_header_and_the_c_compiler(tmp_path, name, T, fields, want):
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    declared = []
    for d in body.split(";"):
        if d.strip():                                        # "float lr, beta1, beta2, eps" declares four
            head, *more = d.split(",")
            declared += [re.findall(r"([A-Za-z_]\w*)\s*(?:\[\d+\])?\s*$", head.strip())[0]] + [m.strip() for m in more]
    T = getattr(_lib, T)
    assert declared == [f[0] for f in T._fields_] == fields
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("' + "%zu " * (len(fields) + 1) + '\\n", '
                 f"sizeof({name}), " + ", ".join(f"offsetof({name}, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(c), "-o", str(exe)])
    got = [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == got == want


# ---- the rules ----------------------------------------------------------------------------------------------------------------
def _rays(_lib, **null):
    r = _lib.RayGradients()
    for f in RAY_FIELDS:
        setattr(r, f, None if null.get(f) else P)
    return r


def _pose(_lib, n_images=3, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15, buffers=True):
    p = _lib.PoseRefinement()
    p.n_images, p.lr, p.beta1, p.beta2, p.eps = n_images, lr, beta1, beta2, eps
    if buffers:
        for f in ("poses0", "poses", "delta", "m", "v", "steps", "grad", "drawn"):
            setattr(p, f, P)
    return p


def _args(_lib, grid=True, trace_mode=1):
    a = _lib.TrainStepArgs()
    a.batch.vr_mode, a.batch.sample_type = 1, 3
    a.batch.mlp, a.batch.grid = P, (P if grid else None)
    a.trace.mode = trace_mode
    a.trace.rays_d = P
    return a


def _step(_lib, args, rays, pose=None, reg=None):
    lib = _lib.lib()
    rc = lib.rtxn_train_step_rays(C.byref(args), None, None, None, C.byref(reg) if reg is not None else None, None, None, None,
                                  C.byref(rays) if rays is not None else None, C.byref(pose) if pose is not None else None, None)
    return rc, lib.rtxn_last_error()


def test_a_model_without_a_hash_grid_is_refused():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_ray_gradients_supported(P, None) == 0 and lib.rtxn_ray_gradients_supported(None, P) == 0
    assert lib.rtxn_ray_gradients_supported(P, P) == 1
    rc, msg = _step(_lib, _args(_lib, grid=False), _rays(_lib))
    assert rc == 1 and b"rtxn_train_step_rays" in msg and b"rays" in msg and b"hash grid" in msg, msg
    b = _args(_lib, grid=False).batch
    assert lib.rtxn_train_gradients_rays(C.byref(b), None, None, None, None, None, C.byref(_rays(_lib)), None) == 1
    msg = lib.rtxn_last_error()
    assert b"rtxn_train_gradients_rays" in msg and b"hash grid" in msg, msg


@pytest.mark.parametrize("field", RAY_FIELDS)
def test_a_null_among_the_six_buffers_is_refused_by_name(field):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    rc, msg = _step(_lib, _args(_lib), _rays(_lib, **{field: True}))
    assert rc == 1 and f"rays->{field} is NULL".encode() in msg, msg
    b = _args(_lib).batch
    assert lib.rtxn_train_gradients_rays(C.byref(b), None, None, None, None, None, C.byref(_rays(_lib, **{field: True})), None) == 1
    assert f"rtxn_train_gradients_rays: rays->{field} is NULL".encode() in lib.rtxn_last_error()


def test_pose_without_rays_compat_traversal_and_foreign_regulariser_buffers_are_refused():
    from rtx_nerf_amd import _lib
    rc, msg = _step(_lib, _args(_lib), None, _pose(_lib))
    assert rc == 1 and b"pose without rays" in msg, msg
    rc, msg = _step(_lib, _args(_lib, trace_mode=0), _rays(_lib))
    assert rc == 1 and b"trace.mode = 0" in msg and b"RTXN_TRACE_DDA" in msg, msg
    reg = _lib.TrainRegularizer()
    reg.distortion_weight, reg.t_start, reg.t_end, reg.distortion = 0.01, C.c_void_p(8192), C.c_void_p(8192), P
    rc, msg = _step(_lib, _args(_lib), _rays(_lib), reg=reg)
    assert rc == 1 and b"same buffers" in msg, msg
    reg.t_start = reg.t_end = P                                  # shared: accepted, the call fails later on the batch's own checks
    rc, msg = _step(_lib, _args(_lib), _rays(_lib), reg=reg)
    assert rc == 1 and b"batch.n_rays" in msg, msg
    p = _pose(_lib)
    p.drawn = None
    rc, msg = _step(_lib, _args(_lib), _rays(_lib), p)
    assert rc == 1 and b"pose->drawn" in msg, msg


_BAD_POSE = [("lr", dict(lr=-1e-3)), ("lr", dict(lr=float("nan"))), ("lr", dict(lr=float("inf"))), ("beta1", dict(beta1=1.0)),
             ("beta1", dict(beta1=-0.1)), ("beta1", dict(beta1=float("nan"))), ("beta2", dict(beta2=1.0)), ("beta2", dict(beta2=1.5)),
             ("eps", dict(eps=0.0)), ("eps", dict(eps=-1e-15)), ("eps", dict(eps=float("inf"))), ("n_images", dict(n_images=0))]


@pytest.mark.parametrize("field,kw", _BAD_POSE, ids=[f"{f}={list(k.values())[0]}" for f, k in _BAD_POSE])
def test_every_surface_refuses_a_pose_rule_by_name(field, kw):
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    p = _pose(_lib, **kw)
    surfaces = [("rtxn_pose_refinement_check", lib.rtxn_pose_refinement_check(C.byref(p)), lib.rtxn_last_error()),
                ("rtxn_pose_gradients", lib.rtxn_pose_gradients(P, P, P, P, 4, C.byref(p), None), lib.rtxn_last_error()),
                ("rtxn_pose_step", lib.rtxn_pose_step(C.byref(p), None), lib.rtxn_last_error()),
                ("rtxn_pose_compose", lib.rtxn_pose_compose(C.byref(p), None), lib.rtxn_last_error())]
    rc, msg = _step(_lib, _args(_lib), _rays(_lib), p)
    surfaces.append(("rtxn_train_step_rays", rc, msg))
    for name, rc, msg in surfaces:
        assert rc == 1 and f"pose->{field}".encode() in msg and name.encode() in msg, (name, rc, msg)
    with pytest.raises(_lib.RtxnError, match=field):
        api.pose_refinement(**{"n_images": 3, **kw})


def test_valid_structs_reach_the_arguments_own_checks_and_null_the_calls_without_them():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    assert lib.rtxn_pose_refinement_check(C.byref(_pose(_lib, buffers=False))) == 0
    assert lib.rtxn_pose_refinement_check(C.byref(_pose(_lib, lr=0.0, beta1=0.0, beta2=0.0, buffers=False))) == 0     # lr = 0 is a valid run
    assert lib.rtxn_pose_step(C.byref(_pose(_lib, buffers=False)), None) == 1 and b"NULL among poses0" in lib.rtxn_last_error()
    assert lib.rtxn_pose_gradients(None, P, P, P, 4, C.byref(_pose(_lib)), None) == 1 and b"drawn" in lib.rtxn_last_error()
    assert lib.rtxn_pose_gradients(P, P, P, P, 0, C.byref(_pose(_lib)), None) == 1 and b"n_rays = 0" in lib.rtxn_last_error()
    rc, msg = _step(_lib, _args(_lib), _rays(_lib), _pose(_lib))
    assert rc == 1 and b"batch.n_rays" in msg, msg                 # both accepted: the step's own checks come next
    assert lib.rtxn_train_step_rays(None, None, None, None, None, None, None, None, None, None, None) == 1
    assert b"rtxn_train_step_reg: NULL arguments" in lib.rtxn_last_error()          # NULL, NULL: the call that existed before
    assert lib.rtxn_train_gradients_rays(None, None, None, None, None, None, None, None) == 1
    assert b"rtxn_train_gradients_reg: NULL batch" in lib.rtxn_last_error()
    assert lib.rtxn_hashgrid_input_gradient_segments(None, P, P, P, 4, 3, P, None, None, 1.0, None, P, P, None) == 1
    assert b"rtxn_hashgrid_input_gradient_segments: NULL grid" in lib.rtxn_last_error()
    assert lib.rtxn_ray_gradients_reduce(P, P, P, P, P, P, -1, P, P, None) == 1 and b"n_rays = -1" in lib.rtxn_last_error()
    p = api.pose_refinement(5, lr=2e-3)
    assert p.n_images == 5 and abs(p.lr - 2e-3) < 1e-9 and abs(p.eps - 1e-15) < 1e-21 and not p.poses0


def test_input_gradient_refuses_bad_sampling_and_unscale():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    hg = api.HashGrid(2, 2, 12, 8, 2.0)
    assert lib.rtxn_hashgrid_input_gradient_segments(hg._h, P, P, P, 4, 4, P, None, None, 1.0, None, P, P, None) == 1      # type 4 needs a jitter
    assert b"rtxn_hashgrid_input_gradient_segments" in lib.rtxn_last_error()
    assert lib.rtxn_hashgrid_input_gradient_segments(hg._h, P, P, P, -1, 3, P, None, None, 1.0, None, P, P, None) == 1
    assert b"n_segments = -1" in lib.rtxn_last_error()
    assert lib.rtxn_hashgrid_input_gradient_segments(hg._h, P, P, P, 4, 3, P, None, None, float("nan"), None, P, P, None) == 1
    assert b"unscale" in lib.rtxn_last_error()
    assert lib.rtxn_hashgrid_input_gradient_segments(hg._h, P, P, P, 4, 3, P, C.c_void_p(4100), None, 1.0, None, P, P, None) == 1
    assert b"live_ws" in lib.rtxn_last_error()


# ---- the Trainer ----------------------------------------------------------------------------------------------------------------
def test_trainer_refuses_before_allocating():
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match="ray_gradients"):
        Trainer(16, None, encoding="freq", device="cpu", ray_gradients=True)
    images = types.SimpleNamespace(channels=3, n_images=2)
    t = Trainer.__new__(Trainer)
    t.target_channels, t.ray_gradients, t.image_set = 3, False, None
    with pytest.raises(ValueError, match="ray_gradients=True"):
        t.attach_images(images, refine_poses=True)
    t.ray_gradients = True
    for bad, what in (({"lr": -1.0}, "lr"), ({"beta1": 1.0}, "beta1"), ({"eps": 0.0}, "eps"), ({"rate": 1.0}, "rate"), ("yes", "refine_poses")):
        with pytest.raises(ValueError, match=what):
            t.attach_images(images, refine_poses=bad)
    with pytest.raises(ValueError, match="prefetch"):
        t.capture_step(16, prefetch=True)
