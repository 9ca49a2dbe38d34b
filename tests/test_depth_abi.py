"""CPU-side checks of depth supervision at the C-ABI boundary (rtxn_train_depth, rtxn_volrender_depth_train,
rtxn_train_gradients_depth, rtxn_train_step_depth, rtxn_depth_targets): symbols and bindings, the structs' layout
against the C compiler, every rule the entry points check before any device is touched, and the name rule of DESIGN 5.17 over
NULL and inactive structs.  The Trainer's and the ImageSet's own refusals are checked here too (they raise before allocating)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_volrender_depth_train", "rtxn_train_gradients_depth", "rtxn_train_step_depth", "rtxn_depth_targets",
               "rtxn_load_png_gray16", "rtxn_free_png_gray16")
VR_COMPAT, VR_NERF = 0, 1
REGULAR, MIDPOINT_WORLD, JITTER_WORLD = 0, 3, 4
TRACE_COMPAT, TRACE_DDA = 0, 1
L2, L1, HUBER, RELATIVE_L2 = 0, 1, 2, 3
P, Q = C.c_void_p(4096), C.c_void_p(8192)           # fake device pointers: never launched from here
FIELDS = ["weight", "kind", "param", "target", "t_start", "t_end", "depth", "depth_loss"]
TARGET_FIELDS = ["depth", "poses", "n_images", "width", "height", "format", "kind", "scale", "n_rays", "drawn", "rays_d", "target"]


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_depth_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    assert lib.rtxn_version() == 100


@pytest.mark.parametrize("name,cls,fields,want", [("rtxn_train_depth", "TrainDepth", FIELDS, [56, 0, 4, 8, 16, 24, 32, 40, 48]),
                                                  ("rtxn_depth_targets_args", "DepthTargetsArgs", TARGET_FIELDS,
                                                   [72, 0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56, 64])])
def test_struct_layouts_match_the_header_and_the_c_compiler(tmp_path, name, cls, fields, want):
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    decl = []
    for d in body.split(";"):
        if d.strip():
            decl += [re.findall(r"([A-Za-z_]\w*)\s*$", part.strip())[0] for part in d.split(",")]
    T = getattr(_lib, cls)
    assert decl == [f[0] for f in T._fields_] == fields
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("' + "%zu " * (len(fields) + 1) + '\\n", '
                 f"sizeof({name}), " + ", ".join(f"offsetof({name}, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f in fields] == want


def _depth(_lib, weight=0.5, kind=L2, param=0.0, target=P, t_start=P, t_end=P, depth=None, depth_loss=None):
    s = _lib.TrainDepth()
    s.weight, s.kind, s.param, s.target, s.t_start, s.t_end, s.depth, s.depth_loss = weight, kind, param, target, t_start, t_end, depth, depth_loss
    return s


def _entries(_lib, depth, vr=VR_NERF, stype=MIDPOINT_WORLD, trace=TRACE_DDA, reg=None, rays=None):
    """(name, return code, message) of the three entry points on an otherwise empty batch: an accepted struct fails later, on the
    batch's own checks, under the entry point it forwards to"""
    lib = _lib.lib()
    batch = _lib.TrainBatch()
    batch.vr_mode, batch.sample_type, batch.mlp, batch.grid = vr, stype, (P if rays is not None else None), (P if rays is not None else None)
    args = _lib.TrainStepArgs()
    args.batch.vr_mode, args.batch.sample_type, args.trace.mode = vr, stype, trace
    args.batch.mlp, args.batch.grid = batch.mlp, batch.grid
    jit = _lib.SampleJitter() if stype == JITTER_WORLD else None
    jp = C.byref(jit) if jit is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    out = [("rtxn_train_gradients_depth", lib.rtxn_train_gradients_depth(C.byref(batch), None, jp, None, ref(reg), None, ref(rays), ref(depth), None),
            lib.rtxn_last_error()),
           ("rtxn_train_step_depth", lib.rtxn_train_step_depth(C.byref(args), None, jp, None, ref(reg), None, None, None, ref(rays), None, None,
                                                               ref(depth), None), lib.rtxn_last_error())]
    if vr == VR_NERF and rays is None:       # the compositor has no mode argument and no rays: it is the NeRF one
        out.append(("rtxn_volrender_depth_train", lib.rtxn_volrender_depth_train(P, P, P, P, 4, 32, P, 128.0, P, P, P, P, None, None, ref(reg),
                                                                                 None, ref(depth), None), lib.rtxn_last_error()))
    return out


_REJECTED = [(dict(weight=-0.5), b"depth->weight"), (dict(weight=float("nan")), b"depth->weight"), (dict(weight=float("inf")), b"depth->weight"),
             (dict(weight=-1.0, target=None, t_start=None, t_end=None), b"depth->weight"),
             (dict(kind=RELATIVE_L2), b"depth->kind"), (dict(kind=7), b"depth->kind"), (dict(weight=0.0, kind=-1), b"depth->kind"),
             (dict(kind=HUBER, param=0.0), b"depth->param"), (dict(kind=HUBER, param=-0.1), b"depth->param"),
             (dict(kind=HUBER, param=float("nan")), b"depth->param"), (dict(kind=HUBER, param=float("inf")), b"depth->param"),
             (dict(target=None), b"depth->target"), (dict(t_start=None), b"depth->t_start"), (dict(t_end=None), b"depth->t_start"),
             (dict(weight=0.0, depth=P, target=None), b"depth->target"), (dict(weight=0.0, depth_loss=P, t_start=None), b"depth->t_start")]


@pytest.mark.parametrize("kw,word", _REJECTED)
def test_depth_entries_reject_bad_structs_before_touching_a_device(kw, word):
    """RTXN_ERR_INVALID (1) and a message naming the field under the entry point's name, with or without a GPU"""
    from rtx_nerf_amd import _lib
    for name, rc, msg in _entries(_lib, _depth(_lib, **kw)):
        assert rc == 1 and word in msg and name.encode() in msg, (name, rc, msg)


@pytest.mark.parametrize("kw", [dict(weight=0.5), dict(weight=0.0, depth=P), dict(weight=0.0, depth_loss=P), dict(kind=HUBER, param=0.1)])
def test_depth_needs_the_nerf_compositor_world_samples_and_the_dda_walk(kw):
    from rtx_nerf_amd import _lib
    for name, rc, msg in _entries(_lib, _depth(_lib, **kw), vr=VR_COMPAT, stype=REGULAR):
        assert rc == 1 and b"RTXN_VR_NERF" in msg and b"depth->weight" in msg and name.encode() in msg, (name, msg)
    for name, rc, msg in _entries(_lib, _depth(_lib, **kw), stype=REGULAR):
        if name != "rtxn_volrender_depth_train":           # the compositor has no sample type
            assert rc == 1 and b"sample_type" in msg and b"RTXN_SAMPLING_MIDPOINT_WORLD" in msg and name.encode() in msg, (name, msg)
    for stype in (MIDPOINT_WORLD, JITTER_WORLD):
        for name, rc, msg in _entries(_lib, _depth(_lib, **kw), stype=stype, trace=TRACE_COMPAT):
            if name == "rtxn_train_step_depth":
                assert rc == 1 and b"trace.mode" in msg and b"RTXN_TRACE_COMPAT" in msg and b"rtxn_train_step_depth" in msg, msg
            elif name == "rtxn_train_gradients_depth":     # accepted: the batch's own checks, under the name they carry
                assert rc == 1 and b"NULL batch or model" in msg, msg


def test_distances_are_shared_with_the_regulariser_and_the_ray_gradients():
    """check_ray_gradients' sentence: the traversal writes t_start / t_end once"""
    from rtx_nerf_amd import _lib
    reg = _lib.TrainRegularizer()
    reg.distortion_weight, reg.t_start, reg.t_end = 0.5, Q, Q
    for name, rc, msg in _entries(_lib, _depth(_lib), reg=reg):
        assert rc == 1 and b"depth->t_start / t_end and reg->t_start / t_end must be the same buffers (the traversal writes them once)" in msg, msg
        assert name.encode() in msg
    reg.t_start, reg.t_end = P, P
    for name, rc, msg in _entries(_lib, _depth(_lib), reg=reg):
        assert b"same buffers" not in msg, msg
    inactive = _lib.TrainRegularizer()               # an inactive regulariser has no distances to share
    inactive.t_start, inactive.t_end = Q, Q
    for name, rc, msg in _entries(_lib, _depth(_lib), reg=inactive):
        assert b"same buffers" not in msg, msg
    rays = _lib.RayGradients()
    for f in ("t_start", "t_end", "dstart", "dend", "d_origin", "d_direction"):
        setattr(rays, f, Q)
    for name, rc, msg in _entries(_lib, _depth(_lib), rays=rays):
        assert rc == 1 and b"rays->t_start / t_end and depth->t_start / t_end must be the same buffers (the traversal writes them once)" in msg, msg
        assert name.encode() in msg


def test_valid_and_inactive_structs_and_the_name_rule():
    """A valid struct passes the rules: the compositor then needs a device (RTXN_ERR_HIP = 2 without one; with one, an empty batch
    is RTXN_OK and touches no buffer), the batch entry points meet the batch's own checks.  The name rule: a rung reports under its
    own name while it holds its struct; with depth == NULL it is the rung below (_cameras -> _rays -> ... -> _reg), and an
    inactive struct runs the rung below's call, whose own checks report under their names."""
    import torch
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    want = 0 if torch.cuda.is_available() else 2
    for d in (_depth(_lib), _depth(_lib, depth=P, depth_loss=P), _depth(_lib, 0.0, depth=P), _depth(_lib, kind=L1), _depth(_lib, kind=HUBER, param=0.1)):
        assert lib.rtxn_volrender_depth_train(P, P, P, P, 0, 32, P, 128.0, P, P, None, P, None, None, None, None, C.byref(d), None) == want
        if want == 2:
            assert b"no HIP device" in lib.rtxn_last_error()
        assert lib.rtxn_volrender_depth_train(P, P, P, P, -1, 32, P, 1.0, P, P, P, P, None, None, None, None, C.byref(d), None) == 1
        assert b"rtxn_volrender_depth_train: batch_size" in lib.rtxn_last_error()
        for stype in (MIDPOINT_WORLD, JITTER_WORLD):
            for name, rc, msg in _entries(_lib, d, stype=stype)[:2]:
                assert rc == 1 and (b"NULL batch or model" in msg or b"batch.mlp is NULL" in msg), (name, msg)
    for d in (None, _depth(_lib, 0.0, target=None, t_start=None, t_end=None), _depth(_lib, 0.0)):
        dp = C.byref(d) if d is not None else None
        assert lib.rtxn_volrender_depth_train(P, P, P, P, -1, 32, P, 1.0, P, P, P, P, None, None, None, None, dp, None) == 1
        assert b"rtxn_volrender_l2_train: batch_size" in lib.rtxn_last_error()
        for name, rc, msg in _entries(_lib, d, vr=VR_COMPAT, stype=REGULAR, trace=TRACE_COMPAT)[:2]:
            assert rc == 1 and (b"NULL batch or model" in msg or b"batch.mlp is NULL" in msg), (name, msg)
    # a malformed struct BELOW the rung: reported under the depth rung's name with the struct, under the rung below's without it
    bad = _lib.TrainLoss()
    bad.kind = 99
    batch, args = _lib.TrainBatch(), _lib.TrainStepArgs()
    batch.vr_mode = args.batch.vr_mode = VR_NERF
    batch.sample_type = args.batch.sample_type = MIDPOINT_WORLD
    args.trace.mode = TRACE_DDA
    for d, grads, step in ((_depth(_lib), b"rtxn_train_gradients_depth:", b"rtxn_train_step_depth:"),
                           (_depth(_lib, 0.0), b"rtxn_train_gradients_depth:", b"rtxn_train_step_depth:"),
                           (None, b"rtxn_train_gradients_reg:", b"rtxn_train_step_reg:")):
        dp = C.byref(d) if d is not None else None
        assert lib.rtxn_train_gradients_depth(C.byref(batch), None, None, C.byref(bad), None, None, None, dp, None) == 1
        assert grads in lib.rtxn_last_error() and b"loss->kind" in lib.rtxn_last_error(), lib.rtxn_last_error()
        assert lib.rtxn_train_step_depth(C.byref(args), None, None, C.byref(bad), None, None, None, None, None, None, None, dp, None) == 1
        assert step in lib.rtxn_last_error() and b"loss->kind" in lib.rtxn_last_error(), lib.rtxn_last_error()
    assert lib.rtxn_train_gradients_depth(None, None, None, None, None, None, None, None, None) == 1 and b"NULL batch" in lib.rtxn_last_error()
    assert lib.rtxn_train_step_depth(None, None, None, None, None, None, None, None, None, None, None, None, None) == 1
    assert b"NULL arguments" in lib.rtxn_last_error()


def _targets(_lib, **kw):
    a = _lib.DepthTargetsArgs()
    a.depth, a.poses, a.n_images, a.width, a.height, a.format, a.kind, a.scale, a.n_rays = P, P, 3, 5, 4, 0, 0, 1e-4, 10
    a.drawn, a.rays_d, a.target = P, P, P
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [(dict(depth=None), b"NULL depth or poses"), (dict(poses=None), b"NULL depth or poses"),
                                     (dict(drawn=None), b"NULL drawn, rays_d or target"), (dict(rays_d=None), b"NULL drawn, rays_d or target"),
                                     (dict(target=None), b"NULL drawn, rays_d or target"), (dict(format=2), b"unknown depth format 2"),
                                     (dict(format=-1), b"unknown depth format"), (dict(kind=2), b"unknown depth kind 2"),
                                     (dict(scale=0.0), b"scale = 0"), (dict(scale=-1.0), b"scale = -1"), (dict(scale=float("nan")), b"scale = nan"),
                                     (dict(scale=float("inf")), b"scale = inf"), (dict(n_images=0), b"n_images = 0"),
                                     (dict(n_rays=0), b"n_rays = 0"), (dict(width=0), b"0 x 4 frames"), (dict(width=8192, height=4096), b"8192 x 4096")])
def test_depth_targets_rejects_bad_arguments_before_touching_a_device(kw, word):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_depth_targets(C.byref(_targets(_lib, **kw)), None) == 1
    assert word in lib.rtxn_last_error() and b"rtxn_depth_targets:" in lib.rtxn_last_error(), lib.rtxn_last_error()
    assert lib.rtxn_depth_targets(None, None) == 1 and b"args is NULL" in lib.rtxn_last_error()


def test_structs_and_signatures_from_python():
    import inspect
    from rtx_nerf_amd import api
    s = api.train_depth()
    assert s.weight == 0.0 and s.kind == L2 and not s.target and not s.t_start and not s.depth and not s.depth_loss
    assert api.train_depth(0.25, "huber").param == pytest.approx(0.1) and api.train_depth(0.25, "l1").kind == L1
    with pytest.raises(ValueError, match="relative_l2"):
        api.train_depth(0.25, "relative_l2")
    for fn in (api.train_gradients, api.train_step, api.volrender_depth_train):
        assert "depth" in inspect.signature(fn).parameters
    assert api._ladder_entry("rtxn_train_step", api._STEP_LADDER, (None,) * 10 + (s,)) == ("rtxn_train_step_depth", 11)
    assert api._ladder_entry("rtxn_train_step", api._STEP_LADDER, (None,) * 9 + (1, None)) == ("rtxn_train_step_cameras", 10)
    assert api._ladder_entry("rtxn_train_gradients", api._GRADIENTS_LADDER, (None,) * 6 + (s,)) == ("rtxn_train_gradients_depth", 7)
    assert api._ladder_entry("rtxn_train_gradients", api._GRADIENTS_LADDER, (None,) * 7) == ("rtxn_train_gradients", 0)


@pytest.mark.parametrize("kw,word", [(dict(depth_weight=-1.0), "depth_weight = -1.0"), (dict(depth_weight=float("nan")), "depth_weight"),
                                     (dict(depth_weight=0.1, mode="compat"), "mode='nerf'"),
                                     (dict(depth_weight=0.1, depth_loss="relative_l2"), "depth_loss 'relative_l2'"),
                                     (dict(depth_weight=0.1, depth_loss="huber", depth_loss_param=0.0), "depth_loss_param")])
def test_trainer_refuses_depth_terms_it_cannot_train(kw, word):
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match=re.escape(word)):
        Trainer(16, None, encoding="freq", device="cpu", **kw)


def test_trainer_refuses_the_depth_term_with_the_three_launch_compositor(monkeypatch):
    from rtx_nerf_amd.train import Trainer
    monkeypatch.setenv("RTXN_TRAIN_FUSE_COMPOSITOR", "0")
    with pytest.raises(ValueError, match="RTXN_TRAIN_FUSE_COMPOSITOR=0"):
        Trainer(16, None, encoding="freq", device="cpu", depth_weight=0.1)


def test_image_set_takes_depth_and_leaves_its_struct_alone():
    """depth is checked and counted; c_struct() is what it was (rtxn_image_set has no depth field)"""
    import torch
    from rtx_nerf_amd import api
    img, poses = torch.zeros((2, 4, 5, 3)), torch.zeros((2, 16))
    plain = api.ImageSet(img, poses, 1.0)
    assert plain.depth is None and plain.nbytes() == 2 * 4 * 5 * 3 * 4 + 2 * 16 * 4
    for dt, size in ((torch.uint16, 2), (torch.float32, 4)):
        s = api.ImageSet(img, poses, 1.0, depth=torch.zeros((2, 4, 5), dtype=dt), depth_unit=1e-3, depth_kind="ray")
        assert s.nbytes() == plain.nbytes() + 2 * 4 * 5 * size and s.depth_kind == "ray" and s.depth_unit == 1e-3
    for bad, word in ((dict(depth=torch.zeros((2, 5, 4))), "depth of shape"), (dict(depth=torch.zeros((2, 4, 5), dtype=torch.int32)), "depth of shape"),
                      (dict(depth=torch.zeros((2, 4, 5)), depth_kind="disparity"), "depth_kind"),
                      (dict(depth=torch.zeros((2, 4, 5)), depth_unit=0.0), "depth_unit")):
        with pytest.raises(ValueError, match=word):
            api.ImageSet(img, poses, 1.0, **bad)
    assert [f[0] for f in api._lib.ImageSet._fields_] == ["images", "poses", "n_images", "width", "height", "channels", "format", "focal_length",
                                                          "aspect_ratio"]
