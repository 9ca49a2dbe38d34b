"""The depth-map loader: rtxn_load_png_gray16 on gray PNGs written here with zlib and struct -- 16 bits plain and
Adam7-interlaced, row filters 0 (None) and 4 (Paeth), 8 bits -- with the values compared exactly; the colour types it refuses;
and loader.read_depth_maps over a transforms.json: both key names, the unit keys, a frame without a depth key, .npy maps, and
the refusals.  No GPU."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))      # x0, y0, dx, dy


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def _scanlines(img, depth, channels, filt):
    """img [h][w][channels] of integer samples -> filtered scanlines (filter 0 or 4 on every row)"""
    h, w = img.shape[:2]
    if h == 0 or w == 0:
        return b""
    bpp = channels * depth // 8
    rows = img.astype(">u2" if depth == 16 else np.uint8).reshape(h, -1).view(np.uint8).reshape(h, w * bpp)
    out, prev = bytearray(), np.zeros(w * bpp, np.int64)
    for y in range(h):
        row = rows[y].astype(np.int64)
        out.append(filt)
        for i in range(w * bpp):
            a, b, c = (row[i - bpp] if i >= bpp else 0), prev[i], (prev[i - bpp] if i >= bpp else 0)
            out.append(int(row[i] - (_paeth(a, b, c) if filt == 4 else 0)) & 255)
        prev = row
    return bytes(out)


def write_png(path, img, depth, ctype=0, interlace=False, filt=0):
    """img [h][w] (gray) or [h][w][channels]; ctype: 0 gray, 2 RGB, 4 gray + alpha, 6 RGBA"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, ch = img.shape
    if interlace:
        raw = b"".join(_scanlines(img[y0::dy, x0::dx], depth, ch, filt) for x0, y0, dx, dy in ADAM7)
    else:
        raw = _scanlines(img, depth, ch, filt)
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1 if interlace else 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw)) + _chunk(b"IEND", b""))


@pytest.mark.parametrize("depth,interlace,filt", [(16, False, 0), (16, False, 4), (16, True, 0), (16, True, 4), (8, False, 0), (8, False, 4),
                                                  (8, True, 4)])
def test_gray_png_loads_to_its_values_exactly(tmp_path, depth, interlace, filt):
    from rtx_nerf_amd import loader
    rng = np.random.default_rng(depth + 2 * interlace + filt)
    v = rng.integers(0, 1 << depth, (11, 13)).astype(np.uint16)
    v[0, 0], v[-1, -1], v[3, 4] = 0, (1 << depth) - 1, 0x0102 & ((1 << depth) - 1)      # both bytes of a 16-bit sample matter
    write_png(tmp_path / "d.png", v, depth, interlace=interlace, filt=filt)
    got = loader.load_png_gray16(tmp_path / "d.png")
    assert got.dtype == np.uint16 and got.shape == (11, 13) and np.array_equal(got, v)      # 8 bits: v, not v * 257


@pytest.mark.parametrize("ctype,channels,depth", [(2, 3, 8), (2, 3, 16), (6, 4, 8), (4, 2, 16), (4, 2, 8)])
def test_other_colour_types_are_refused_with_a_message(tmp_path, ctype, channels, depth):
    from rtx_nerf_amd import _lib, loader
    write_png(tmp_path / "c.png", np.random.default_rng(1).integers(0, 200, (5, 6, channels)), depth, ctype=ctype)
    with pytest.raises(_lib.RtxnError, match=f"colour type {ctype} with {depth} bits: a depth map is a gray PNG"):
        loader.load_png_gray16(tmp_path / "c.png")


def test_unreadable_files_are_refused(tmp_path):
    from rtx_nerf_amd import _lib, loader
    with pytest.raises(_lib.RtxnError, match="cannot read the file"):
        loader.load_png_gray16(tmp_path / "missing.png")
    (tmp_path / "junk.png").write_bytes(b"not a png at all")
    with pytest.raises(_lib.RtxnError, match="not a PNG"):
        loader.load_png_gray16(tmp_path / "junk.png")
    good = tmp_path / "good.png"
    write_png(good, np.arange(30).reshape(5, 6), 16)
    (tmp_path / "short.png").write_bytes(good.read_bytes()[:60])
    with pytest.raises(_lib.RtxnError, match="Failed to load depth map"):
        loader.load_png_gray16(tmp_path / "short.png")


def _scene(tmp_path, frames, **top):
    (tmp_path / "depth").mkdir(exist_ok=True)
    path = tmp_path / "transforms.json"
    path.write_text(json.dumps(dict(top, frames=frames)))
    return path


def test_read_depth_maps_reads_both_keys_and_zero_fills_a_frame_without_one(tmp_path):
    from rtx_nerf_amd import loader
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 65536, (4, 5)).astype(np.uint16), rng.integers(0, 256, (4, 5)).astype(np.uint16)
    path = _scene(tmp_path, [{"file_path": "r_0", "depth_file_path": "depth/a.png"}, {"file_path": "r_1"},
                             {"file_path": "r_2", "depth_path": "depth/b"}])
    write_png(tmp_path / "depth" / "a.png", a, 16, interlace=True, filt=4)
    write_png(tmp_path / "depth" / "b.png", b, 8)                    # named without its extension, as instant-ngp's file_path may be
    depth, unit = loader.read_depth_maps(path, 5, 4)
    assert depth.dtype == np.uint16 and depth.shape == (3, 4, 5) and unit == 1e-3
    assert np.array_equal(depth[0], a) and not depth[1].any() and np.array_equal(depth[2], b)


def test_read_depth_maps_units(tmp_path):
    from rtx_nerf_amd import loader
    frames = [{"depth_file_path": "depth/a.png"}]
    write_png(tmp_path / "depth_a.png", np.ones((2, 2)), 16)
    (tmp_path / "depth").mkdir()
    write_png(tmp_path / "depth" / "a.png", np.ones((2, 2)), 16)
    assert loader.read_depth_maps(_scene(tmp_path, frames), 2, 2)[1] == 1e-3
    assert loader.read_depth_maps(_scene(tmp_path, frames, depth_unit_scale_factor=0.25), 2, 2)[1] == 0.25
    assert loader.read_depth_maps(_scene(tmp_path, frames, depth_unit_scale_factor=0.25, integer_depth_scale=0.002), 2, 2)[1] == 0.002
    for bad in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="depth unit"):
            loader.read_depth_maps(_scene(tmp_path, frames, integer_depth_scale=bad), 2, 2)


def test_read_depth_maps_takes_float32_npy_maps(tmp_path):
    from rtx_nerf_amd import loader
    m = np.random.default_rng(4).uniform(0, 7, (4, 5)).astype(np.float32)
    path = _scene(tmp_path, [{"depth_file_path": "depth/m.npy"}, {}])
    np.save(tmp_path / "depth" / "m.npy", m)
    depth, unit = loader.read_depth_maps(path, 5, 4)
    assert depth.dtype == np.float32 and np.array_equal(depth[0], m) and not depth[1].any() and unit == 1.0
    np.save(tmp_path / "depth" / "d.npy", m.astype(np.float64))
    with pytest.raises(ValueError, match=r"frame 0 \(depth/d.npy\).*float32"):
        loader.read_depth_maps(_scene(tmp_path, [{"depth_file_path": "depth/d.npy"}]), 5, 4)
    write_png(tmp_path / "depth" / "p.png", np.ones((4, 5)), 16)
    with pytest.raises(ValueError, match="PNG and .npy depth maps in one set"):
        loader.read_depth_maps(_scene(tmp_path, [{"depth_file_path": "depth/m.npy"}, {"depth_file_path": "depth/p.png"}]), 5, 4)


def test_read_depth_maps_refusals_name_the_frame(tmp_path):
    from rtx_nerf_amd import _lib, loader
    (tmp_path / "depth").mkdir()
    write_png(tmp_path / "depth" / "ok.png", np.ones((4, 5)), 16)
    write_png(tmp_path / "depth" / "small.png", np.ones((3, 5)), 16)
    write_png(tmp_path / "depth" / "rgb.png", np.ones((4, 5, 3)), 8, ctype=2)
    with pytest.raises(ValueError, match=r"frame 1 \(depth/small.png\): the depth map is 5 x 3, the frames are 5 x 4"):
        loader.read_depth_maps(_scene(tmp_path, [{"depth_file_path": "depth/ok.png"}, {"depth_file_path": "depth/small.png"}]), 5, 4)
    with pytest.raises(ValueError, match="no frame has a depth_file_path or depth_path"):
        loader.read_depth_maps(_scene(tmp_path, [{"file_path": "r_0"}, {"file_path": "r_1"}]), 5, 4)
    with pytest.raises(_lib.RtxnError, match="rgb.png: colour type 2"):
        loader.read_depth_maps(_scene(tmp_path, [{"depth_path": "depth/rgb.png"}]), 5, 4)
