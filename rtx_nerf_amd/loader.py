"""Host mirror of loader/data_loader.h over the C ABI (rtxn_load_images_json):
load_images_json / load_synthetic_data / load_data with the reference's names and
behaviour (loader/data_loader.cpp:34-149), returning numpy arrays instead of raw pointers."""
import ctypes as C
import sys

import numpy as np

from . import _lib

RTXN_LOAD_RGBA = 4     # flags bit 2: float[n,H,W,4] straight RGBA (alpha a/255, 1 without alpha); not with bit 0

SYNTHETIC_NAMES = {"CHAIR": "chair/", "DRUMS": "drums/", "FICUS": "ficus/", "HOTDOG": "hotdog/", "LEGO": "lego/",
                   "MATERIALS": "fern/",   # sic: data_loader.cpp:128-130 (quirk Q12)
                   "MIC": "mic/", "SHIP": "ship/"}


class ImageDataset:
    """loader/data_loader.h:20-27: images float[n,H,W,channels] (3, or 4 with RTXN_LOAD_RGBA), poses float[n,16], focal, width,
    height, channels."""

    def __init__(self, images, poses, focal, width, height, channels, camera_angle_x=0.0):
        self.images, self.poses, self.focal = images, poses, focal
        self.image_width, self.image_height, self.image_channels = width, height, channels
        self.camera_angle_x = camera_angle_x


def load_images_json(basename, s, flags=0):
    """data_loader.cpp:34-94.  A missing JSON exits the process as the reference does (:36-39); a frame
    that fails to load returns an empty dataset (:74-78)."""
    d = _lib.ImageDataset()
    rc = _lib.lib().rtxn_load_images_json(str(basename).encode(), s.encode(), flags, C.byref(d))
    if rc != 0:
        msg = _lib.lib().rtxn_last_error().decode()
        print(msg, file=sys.stderr)
        if "transform JSON" in msg:
            sys.exit(1)
        return ImageDataset(np.zeros((0, 0, 0, 3), np.float32), np.zeros((0, 16), np.float32), 0.0, 0, 0, 0)
    n, w, h = d.n_images, d.image_width, d.image_height
    ch = d.image_channels or 3           # 4 with RTXN_LOAD_RGBA (flags bit 2)
    images = np.ctypeslib.as_array(d.images, shape=(n, h, w, ch)).copy() if n else np.zeros((0, h, w, ch), np.float32)
    poses = np.ctypeslib.as_array(d.poses, shape=(n, 16)).copy() if n else np.zeros((0, 16), np.float32)
    out = ImageDataset(images, poses, d.focal, w, h, d.image_channels, d.camera_angle_x)
    _lib.lib().rtxn_free_image_dataset(C.byref(d))
    return out


def load_synthetic_data(directory, flags=0):
    """data_loader.cpp:96-107: only the first split ("train") is loaded (the `break` at :103)."""
    datasets = []
    for split in ("train", "val", "test"):
        datasets.append(load_images_json(directory, split, flags))
        break
    return datasets


def load_llff_data(directory, factor=8, flags=0):
    """Fills the reference's LLFF stub (data_loader.cpp:140-142 sets the directory and returns nothing): poses_bounds.npy
    + the PNG frames of images_<factor>/ -> [ImageDataset] with `.bounds` float[n,2] (near, far); [] when the scene is
    absent or unreadable, which is what the reference returns for every LLFF request."""
    d = _lib.ImageDataset()
    b = C.POINTER(C.c_float)()
    rc = _lib.lib().rtxn_load_llff(str(directory).encode(), int(factor), flags, C.byref(d), C.byref(b))
    if rc != 0:
        print(_lib.lib().rtxn_last_error().decode(), file=sys.stderr)
        return []
    n, w, h = d.n_images, d.image_width, d.image_height
    ch = d.image_channels or 3           # 4 with RTXN_LOAD_RGBA (flags bit 2)
    images = np.ctypeslib.as_array(d.images, shape=(n, h, w, ch)).copy() if n else np.zeros((0, h, w, ch), np.float32)
    poses = np.ctypeslib.as_array(d.poses, shape=(n, 16)).copy() if n else np.zeros((0, 16), np.float32)
    out = ImageDataset(images, poses, d.focal, w, h, d.image_channels, d.camera_angle_x)
    out.bounds = np.ctypeslib.as_array(b, shape=(n, 2)).copy() if n else np.zeros((0, 2), np.float32)
    _lib.lib().rtxn_free_llff_bounds(b)
    _lib.lib().rtxn_free_image_dataset(C.byref(d))
    return [out]


def load_data(scene_type, name, root="./data", flags=0, llff_factor=8):
    """data_loader.cpp:109-149.  scene_type: "SYNTHETIC" | "LLFF".  The reference stops at the directory name for LLFF
    (:140-142) and returns []; here the scene is loaded when it exists (load_llff_data) and [] is returned otherwise."""
    filename = SYNTHETIC_NAMES[name]
    if scene_type == "SYNTHETIC":
        return load_synthetic_data(f"{root}/nerf_synthetic/{filename}", flags)
    return load_llff_data(f"{root}/nerf_llff_data/{filename}", llff_factor, flags)


_CAMERA_KEYS = ("camera_model", "is_fisheye", "fl_x", "fl_y", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2", "w", "h", "camera_angle_x")
_CAMERA_MODEL_NAMES = {"PINHOLE": "pinhole", "SIMPLE_PINHOLE": "pinhole", "OPENCV": "opencv", "OPENCV_FISHEYE": "opencv_fisheye"}


def read_cameras(json_path, width, height):
    """The intrinsics of an instant-ngp / nerfstudio transforms.json for frames loaded at width x height: (model, params), model
    "pinhole" | "opencv" | "opencv_fisheye" and params float32 [n, 12] rows of api.camera_params() -- what api.camera_set() takes.
    Keys camera_model, fl_x, fl_y, cx, cy, k1..k4, p1, p2, w, h, read at the top level and, where a frame carries its own, per
    frame (a frame's key wins): n = 1 when no frame does, else one row per frame in file order.  fl_y defaults to fl_x, cx / cy to
    w / 2, h / 2, w / h to width / height; intrinsics given for w x h are rescaled to the loaded size (fx, cx by width / w;
    fy, cy by height / h); distortion coefficients act on normalised coordinates and are kept.  Without camera_model:
    opencv_fisheye with instant-ngp's is_fisheye, opencv with any non-zero coefficient, else pinhole; the set has ONE model, so
    frames that disagree are refused.  Without fl_x: a centred pinhole from camera_angle_x, the HORIZONTAL field of view,
    fx = fy = width / (2 tan(camera_angle_x / 2)).  cy counts rows of the frame as it is stored; the pose convention is the
    caller's (include/rtxn.h: +y along pose column 1 with py).  Host only; the C loader is not involved."""
    import json
    import math
    with open(json_path) as f:
        top = json.load(f)
    frames = top.get("frames") or []
    per_frame = any(k in fr for fr in frames for k in _CAMERA_KEYS)
    rows, models = [], set()
    for fr in (frames if per_frame else [{}]):
        g = {k: top[k] for k in _CAMERA_KEYS if k in top}
        g.update({k: fr[k] for k in _CAMERA_KEYS if k in fr})
        w, h = float(g.get("w", width)), float(g.get("h", height))
        sx, sy = float(width) / w, float(height) / h
        if "fl_x" in g:
            fx, fy = float(g["fl_x"]) * sx, float(g.get("fl_y", g["fl_x"])) * sy
        elif "camera_angle_x" in g:
            fx = fy = 0.5 * float(width) / math.tan(0.5 * float(g["camera_angle_x"]))
        else:
            raise ValueError(f"read_cameras: {json_path}: neither fl_x nor camera_angle_x")
        cx, cy = float(g.get("cx", 0.5 * w)) * sx, float(g.get("cy", 0.5 * h)) * sy
        k = {n: float(g.get(n, 0.0)) for n in ("k1", "k2", "k3", "k4", "p1", "p2")}
        if "camera_model" in g:
            name = str(g["camera_model"]).upper()
            if name not in _CAMERA_MODEL_NAMES:
                raise ValueError(f"read_cameras: {json_path}: camera_model {g['camera_model']!r}: one of {sorted(_CAMERA_MODEL_NAMES)}")
            model = _CAMERA_MODEL_NAMES[name]
        elif g.get("is_fisheye"):
            model = "opencv_fisheye"
        else:
            model = "opencv" if any(k.values()) else "pinhole"
        models.add(model)
        rows.append([fx, fy, cx, cy, k["k1"], k["k2"], k["k3"], k["k4"], k["p1"], k["p2"], 0.0, 0.0])
    if models == {"pinhole", "opencv"}:        # frames without coefficients under a distorted set: opencv with zeros is the pinhole
        models = {"opencv"}
    if len(models) != 1:
        raise ValueError(f"read_cameras: {json_path}: frames of different camera models {sorted(models)}: one model per set")
    return models.pop(), np.asarray(rows, dtype=np.float32)


def load_png_gray16(path):
    """rtxn_load_png_gray16: a gray PNG of 8 or 16 bits as uint16 [H, W] in the file's own unit (16-bit samples whole, 8-bit
    samples as v); any other colour type raises _lib.RtxnError with the loader's message."""
    w, h, v = C.c_int(), C.c_int(), C.POINTER(C.c_uint16)()
    _lib.check(_lib.lib().rtxn_load_png_gray16(str(path).encode(), C.byref(w), C.byref(h), C.byref(v)), "rtxn_load_png_gray16")
    out = np.ctypeslib.as_array(v, shape=(h.value, w.value)).copy()
    _lib.lib().rtxn_free_png_gray16(v)
    return out


_DEPTH_KEYS = ("depth_file_path", "depth_path")      # nerfstudio; instant-ngp


def read_depth_maps(json_path, width, height):
    """The per-frame depth maps of an instant-ngp / nerfstudio transforms.json for frames loaded at width x height:
    (depth, unit) -- what api.ImageSet(depth=, depth_unit=) takes.  Each frame's depth_file_path (nerfstudio) or depth_path
    (instant-ngp), relative to the JSON, names a gray PNG of 16 or 8 bits (load_png_gray16) or a float32 .npy of shape [H, W];
    depth is uint16 [N, H, W] for PNGs and float32 [N, H, W] for .npy maps (one kind per set), frames in file order.  A frame
    without a depth key gets an all-zero map: no target anywhere in it.  unit: the length of one map unit in the poses' unit --
    the top-level integer_depth_scale (instant-ngp) if present, else depth_unit_scale_factor (nerfstudio), else 1e-3
    (millimetres) for PNGs and 1.0 for .npy maps.  Refused (ValueError): no frame with a depth key, a map whose size is not
    width x height (the frame is named), PNG and .npy maps in one set, a unit that is not finite and > 0.  Host only."""
    import json
    import os
    with open(json_path) as f:
        top = json.load(f)
    frames = top.get("frames") or []
    base = os.path.dirname(os.path.abspath(json_path))
    maps, kinds = [], set()
    for i, fr in enumerate(frames):
        name = next((fr[k] for k in _DEPTH_KEYS if k in fr), None)
        if name is None:
            maps.append(None)
            continue
        path = os.path.join(base, str(name))
        if not os.path.exists(path) and os.path.exists(path + ".png"):
            path += ".png"
        if path.endswith(".npy"):
            m = np.load(path, allow_pickle=False)
            if m.dtype != np.float32:
                raise ValueError(f"read_depth_maps: frame {i} ({name}): a .npy depth map must be float32, got {m.dtype}")
            kinds.add("npy")
        else:
            m = load_png_gray16(path)
            kinds.add("png")
        if m.shape != (int(height), int(width)):
            raise ValueError(f"read_depth_maps: frame {i} ({name}): the depth map is {m.shape[-1]} x {m.shape[0]}, "
                             f"the frames are {width} x {height}")
        maps.append(m)
    if not kinds:
        raise ValueError(f"read_depth_maps: {json_path}: no frame has a depth_file_path or depth_path")
    if len(kinds) != 1:
        raise ValueError(f"read_depth_maps: {json_path}: PNG and .npy depth maps in one set")
    dtype = np.uint16 if kinds == {"png"} else np.float32
    unit = float(top.get("integer_depth_scale", top.get("depth_unit_scale_factor", 1e-3 if dtype == np.uint16 else 1.0)))
    if not (unit > 0.0 and np.isfinite(unit)):
        raise ValueError(f"read_depth_maps: {json_path}: depth unit {unit} (finite, > 0)")
    depth = np.zeros((len(frames), int(height), int(width)), dtype)
    for i, m in enumerate(maps):
        if m is not None:
            depth[i] = m
    return depth, unit


def write_png(path, rgb_float):
    """Rendered frame float[H,W,3] in [0,1] -> 8-bit PNG (stb_image_write's unused role, main.cu:19-21)."""
    img = np.ascontiguousarray(np.rint(np.clip(rgb_float, 0.0, 1.0) * 255.0).astype(np.uint8))
    h, w = img.shape[:2]
    _lib.check(_lib.lib().rtxn_write_png_rgb8(str(path).encode(), img.ctypes.data_as(C.c_void_p), w, h), "rtxn_write_png_rgb8")
