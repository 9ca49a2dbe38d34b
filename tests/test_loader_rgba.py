"""The loader's RGBA form (flags bit 2, RTXN_LOAD_RGBA): float[n][H][W][4] with the RGB that the same flags without bit 2
produce and alpha = a/255 (no gamma), 1 for files without alpha; bit 2 with bit 0 (composite over white) is refused.  CPU only:
PNGs written here with PIL."""
import json
import os

import numpy as np
import pytest
from PIL import Image

from rtx_nerf_amd import loader

RGBA = loader.RTXN_LOAD_RGBA


def _scene(tmp, images):
    """one-split synthetic scene of the given PIL images"""
    os.makedirs(tmp / "train", exist_ok=True)
    frames = []
    for i, im in enumerate(images):
        im.save(tmp / "train" / f"r_{i}.png")
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": np.eye(4).tolist()})
    with open(tmp / "transforms_train.json", "w") as f:
        json.dump({"camera_angle_x": 0.69, "frames": frames}, f)


def _images(rng, h=7, w=11):
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    rgba[0, :4, 3] = [0, 1, 254, 255]
    la = rng.integers(0, 256, (h, w, 2), dtype=np.uint8)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    pal = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").quantize(8)
    pal.info["transparency"] = bytes([0, 40, 128, 200, 255, 7, 99, 255])         # palette with a tRNS alpha per entry
    idx = np.asarray(pal)
    pal_alpha = np.array([0, 40, 128, 200, 255, 7, 99, 255], np.uint8)[idx]
    return ([Image.fromarray(rgba, "RGBA"), Image.fromarray(la, "LA"), Image.fromarray(rgb, "RGB"), pal],
            [rgba[..., 3], la[..., 1], np.full((h, w), 255, np.uint8), pal_alpha])


@pytest.mark.parametrize("gamma_flags", [0, 2])
def test_rgba_flag_keeps_rgb_bit_for_bit_and_adds_linear_alpha(tmp_path, gamma_flags):
    ims, alphas = _images(np.random.default_rng(gamma_flags))
    for k, (im, a) in enumerate(zip(ims, alphas)):
        d = tmp_path / f"s{k}"
        _scene(d, [im])
        rgb = loader.load_images_json(str(d), "train", flags=gamma_flags)
        got = loader.load_images_json(str(d), "train", flags=gamma_flags | RGBA)
        assert rgb.image_channels == 3 and got.image_channels == 4, im.mode
        assert got.images.shape == (1, 7, 11, 4) and got.images.dtype == np.float32
        assert np.array_equal(got.images[..., :3].view(np.uint32), rgb.images.view(np.uint32)), im.mode
        want_a = a.astype(np.float32) / np.float32(255.0)
        assert np.array_equal(got.images[0, ..., 3], want_a), im.mode
        assert np.array_equal(got.poses, rgb.poses) and got.focal == rgb.focal


def test_rgba_flag_with_white_compositing_is_refused(tmp_path, capfd):
    ims, _ = _images(np.random.default_rng(3))
    _scene(tmp_path, ims[:1])
    ds = loader.load_images_json(str(tmp_path), "train", flags=RGBA | 1)
    assert ds.images.shape[0] == 0
    assert "RTXN_LOAD_RGBA" in capfd.readouterr().err
    # flags 0..3 are what they were
    assert loader.load_images_json(str(tmp_path), "train", flags=1).images.shape == (1, 7, 11, 3)


def test_llff_rgba_flag(tmp_path, capfd):
    rng = np.random.default_rng(4)
    os.makedirs(tmp_path / "images_8", exist_ok=True)
    pb = np.zeros((2, 17))
    alphas = []
    for i in range(2):
        pb[i, :15] = np.concatenate([np.eye(3), np.zeros((3, 1)), np.array([[72], [96], [80]])], 1).reshape(-1)
        pb[i, 15:] = [1.0, 5.0]
        arr = rng.integers(0, 256, (9, 12, 4), dtype=np.uint8)
        Image.fromarray(arr, "RGBA").save(tmp_path / "images_8" / f"image{i:03d}.png")
        alphas.append(arr[..., 3])
    np.save(tmp_path / "poses_bounds.npy", pb)
    rgb = loader.load_llff_data(str(tmp_path), factor=8)[0]
    got = loader.load_llff_data(str(tmp_path), factor=8, flags=RGBA)[0]
    assert got.images.shape == (2, 9, 12, 4) and got.image_channels == 4
    assert np.array_equal(got.images[..., :3].view(np.uint32), rgb.images.view(np.uint32))
    assert np.array_equal(got.images[..., 3], np.stack(alphas).astype(np.float32) / np.float32(255.0))
    assert loader.load_llff_data(str(tmp_path), factor=8, flags=RGBA | 1) == []
    assert "RTXN_LOAD_RGBA" in capfd.readouterr().err


def test_ray_dataset_keeps_rgba_pixels(tmp_path):
    from rtx_nerf_amd.train import RayDataset
    ims, alphas = _images(np.random.default_rng(5))
    _scene(tmp_path, [ims[0], ims[0]])
    ds = loader.load_images_json(str(tmp_path), "train", flags=RGBA)
    rays, _ = RayDataset.from_images(ds, device="cpu")
    assert tuple(rays.pixels.shape) == (2 * 7 * 11, 4)
    assert np.array_equal(rays.pixels.numpy(), ds.images.reshape(-1, 4))
    assert rays.rays_o.shape[0] == rays.pixels.shape[0]
    ds3 = loader.load_images_json(str(tmp_path), "train")
    assert tuple(RayDataset.from_images(ds3, device="cpu")[0].pixels.shape) == (2 * 7 * 11, 3)
