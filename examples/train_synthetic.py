#!/usr/bin/env python3
"""End-to-end use of the harness on a NeRF-synthetic scene directory (transforms_train.json + PNG frames, the format the
reference's loader expects at ./data/nerf_synthetic/<scene>, loader/data_loader.cpp:144): load -> device ray dataset ->
train (hash-grid or frequency model) with periodic occupancy refresh -> mean held-out PSNR and SSIM (Trainer.evaluate) -> PNG of a
rendered view.
No dataset ships with this image; pass --make-demo to first write a small procedural scene in the same format.

  python examples/train_synthetic.py --data /path/to/lego [--steps 2000] [--encoding hash]
  python examples/train_synthetic.py --make-demo /tmp/demo_scene --data /tmp/demo_scene --steps 400
  python examples/train_synthetic.py --data /path/to/lego --device-batches     (frames resident as RGBA8/RGB8, batches drawn on the device)
  python examples/train_synthetic.py --data /path/to/lego --loss huber --opacity-weight 0.1     (Huber, and the frames' alpha fitted)
  python examples/train_synthetic.py --data /path/to/lego --distortion-weight 0.01 --loss-scale 4096     (mip-NeRF 360's distortion loss)
  python examples/train_synthetic.py --data /path/to/lego --steps 20000 --lr-schedule cosine:20000 --weight-decay 1e-6 --skip-nonfinite
  python examples/train_synthetic.py --data /path/to/lego --steps 20000 --ema-decay 0.99     (held-out PSNR and SSIM of the live and the averaged weights)
  python examples/train_synthetic.py --data /path/to/lego --pose-noise 0.5,0.02 --refine-poses 1e-3     (noisy poses, refined on the device)
  python examples/train_synthetic.py --data /path/to/lego --mesh lego.ply --mesh-resolution 256 --mesh-iso 30     (triangle mesh of the density field)
  python examples/train_synthetic.py --make-demo /tmp/lens --lens opencv:-0.3,0.1,0,0.001,-0.001 --data /tmp/lens     (a demo scene seen through a lens,
      trained and scored with the cameras its transforms_train.json describes; add --assume-pinhole to train the same frames without them)
  python examples/train_synthetic.py --make-demo /tmp/lens --lens opencv:-0.3,0.1,0,0.001,-0.001 --data /tmp/lens \
      --intrinsics-noise focal=0.03,center=1.5 --refine-cameras     (wrong focal length and principal point on load, refined on the device)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from rtx_nerf_amd import api, loader, scenes
from rtx_nerf_amd.train import RayDataset, Trainer, camera_rays


def parse_lens(spec):
    """MODEL:c1,c2,... -> (model, coefficient keywords of api.camera_params): opencv takes k1, k2, k3, p1, p2, opencv_fisheye
    k1, k2, k3, k4; missing ones are 0"""
    model, _, rest = spec.partition(":")
    names = {"opencv": ("k1", "k2", "k3", "p1", "p2"), "opencv_fisheye": ("k1", "k2", "k3", "k4"), "pinhole": ()}
    if model not in names:
        sys.exit(f"--lens {spec}: model one of {sorted(names)}")
    vals = [float(v) for v in rest.split(",") if v.strip()]
    if len(vals) > len(names[model]):
        sys.exit(f"--lens {spec}: {model} takes {', '.join(names[model])}")
    return model, dict(zip(names[model], vals))


def lens_rays(model, row, pose, res):
    """the frame's rays through the lens, from the float64 restatement the tests hold the device to (tests/_camera_float64.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _camera_float64 as F
    o, d = F.camera_rays(F.MODELS[model], np.asarray(row, np.float32), np.asarray(pose, np.float32).reshape(16), res, res)
    return torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy(d.astype(np.float32)).cuda()


def write_png_gray16(path, values):
    """uint16 [H, W] -> a 16-bit gray PNG (filter 0 on every row): what a depth sensor's export looks like"""
    import struct
    import zlib
    v = np.ascontiguousarray(values, dtype=np.uint16)
    h, w = v.shape
    raw = b"".join(b"\0" + v[y].astype(">u2").tobytes() for y in range(h))
    chunk = lambda kind, body: struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw))
                + chunk(b"IEND", b""))


DEMO_DEPTH_UNIT = 1e-3          # the demo's depth maps count thousandths of the poses' unit


def teacher_depth(o, d, pose, res):
    """uint16 [res, res]: the analytic z-depth of the teacher's surface (the sphere of radius 0.5 its density falls off at) along
    every ray, in DEMO_DEPTH_UNIT of the poses' unit (10 per world unit); 0 where the ray misses it"""
    o64, d64 = o.double().cpu().numpy(), d.double().cpu().numpy()
    b = (o64 * d64).sum(1)
    disc = b * b - (o64 * o64).sum(1) + 0.25
    t = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0.0)), 0.0)
    axis = -np.asarray(pose, np.float64).reshape(4, 4)[:3, 2]
    z = t * (d64 @ (axis / np.linalg.norm(axis))) * 10.0 / DEMO_DEPTH_UNIT
    return np.clip(np.rint(np.where(t > 0, z, 0.0)), 0, 65535).astype(np.uint16).reshape(res, res)


def make_demo(path, n_frames=16, res=64, grid=32, lens=None, depth=False):
    """Writes transforms_train.json + PNGs rendered from the analytic teacher field of tools/train_demo.py.  lens: (model,
    coefficients) of parse_lens -- the frames are then rendered through that lens (a centred camera of the same focal length)
    and the JSON carries its intrinsics in the instant-ngp / nerfstudio keys.  depth: also one 16-bit depth PNG per frame
    (teacher_depth) under depth/, named by the frame's depth_file_path, with depth_unit_scale_factor beside the frames."""
    from train_demo import teacher_field
    os.makedirs(os.path.join(path, "train"), exist_ok=True)
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(grid, 0.72)).view(np.int32).copy()).cuda()
    tr = Trainer(grid, occ, encoding="freq", n_neurons=64, n_hidden_layers=2, batch_rays=res * res, max_segments=res * res * 40,
                 density_scale=150.0)
    focal = scenes.lego_focal_length(True)
    frames, intrinsics = [], {}
    if lens is not None:
        model, coeffs = lens
        f_px = focal * res / 2
        row = api.camera_params(f_px, f_px, res / 2, res / 2, **coeffs)
        api.camera_set(model, row, width=res, height=res, device="cpu")           # refuses a lens that is not invertible over the frame
        intrinsics = dict(camera_model=model.upper(), fl_x=f_px, fl_y=f_px, cx=res / 2, cy=res / 2, w=res, h=res, **coeffs)
    for i in range(n_frames):
        pose = scenes.pose_spherical(360.0 * i / n_frames, -20.0 - 20.0 * (i % 3), origin_scale=10.0)
        o, d = camera_rays(pose, focal, res, res) if lens is None else lens_rays(model, row, pose, res)
        img = tr.render_rays(o, d, radiance_fn=teacher_field).reshape(res, res, 3).cpu().numpy()
        loader.write_png(os.path.join(path, "train", f"r_{i}.png"), img)
        frames.append({"file_path": f"./train/r_{i}", "rotation": 0.0, "transform_matrix": pose.tolist()})
        if depth:
            os.makedirs(os.path.join(path, "depth"), exist_ok=True)
            write_png_gray16(os.path.join(path, "depth", f"d_{i}.png"), teacher_depth(o, d, pose, res))
            frames[-1]["depth_file_path"] = f"./depth/d_{i}.png"
    if depth:
        intrinsics["depth_unit_scale_factor"] = DEMO_DEPTH_UNIT
    with open(os.path.join(path, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": scenes.LEGO_CAMERA_ANGLE_X, **intrinsics, "frames": frames}, f)
    return path


def perturb_poses(poses, rot_deg, trans, seed=0):
    """[N, 4, 4] camera-to-world poses, each rotated about a random axis by rot_deg degrees (a left multiplication, the frame the
    refinement corrects in) and moved by `trans` in a random direction; seeded."""
    rng = np.random.default_rng(seed)
    out = np.array(poses, np.float64)
    for p in out:
        axis, step = rng.standard_normal(3), rng.standard_normal(3)
        w = axis / np.linalg.norm(axis) * np.deg2rad(rot_deg)
        K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        th = np.linalg.norm(w)
        Rw = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
        p[:3, :3] = Rw @ p[:3, :3]
        p[:3, 3] += step / np.linalg.norm(step) * trans
    return out.astype(np.float32)


def parse_groups(spec, names, what):
    """'a=1,b=2' -> {a: 1.0, b: 2.0} over the given names"""
    out = {}
    for part in (p for p in spec.split(",") if p.strip()):
        k, _, v = part.partition("=")
        if k.strip() not in names or not v:
            sys.exit(f"{what} {spec}: entries NAME=VALUE with NAME one of {', '.join(names)}")
        out[k.strip()] = float(v)
    return out


def perturb_cameras(P, focal, center, seed=0):
    """[n, 12] camera rows with fx and fy each scaled by a seeded factor of exp(+-focal) and the principal point moved by
    `center` pixels in a seeded direction"""
    rng = np.random.default_rng(seed)
    out = np.array(P, np.float64)
    for row in out:
        row[:2] *= np.exp(focal * rng.choice([-1.0, 1.0], 2))
        step = rng.standard_normal(2)
        row[2:4] += step / np.linalg.norm(step) * center
    return out.astype(np.float32)


def camera_errors(P, true_P):
    """(mean |log(f / f_true)| over fx and fy, mean principal-point distance in pixels) between two sets of rows"""
    a, b = np.asarray(P, np.float64).reshape(-1, 12), np.asarray(true_P, np.float64).reshape(-1, 12)
    return float(np.abs(np.log(a[:, :2] / b[:, :2])).mean()), float(np.linalg.norm(a[:, 2:4] - b[:, 2:4], axis=1).mean())


def pose_errors(poses, true_poses):
    """(mean rotation angle in degrees, mean translation distance) between two sets of [N, 4, 4] poses"""
    a, b = np.asarray(poses, np.float64).reshape(-1, 4, 4), np.asarray(true_poses, np.float64).reshape(-1, 4, 4)
    cos = (np.einsum("nij,nij->n", a[:, :3, :3], b[:, :3, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))).mean()), float(np.linalg.norm(a[:, :3, 3] - b[:, :3, 3], axis=1).mean())


# --mesh-iso's default: a judgement call from the sweep of DESIGN 5.19 on the --make-demo scene, not derived
DEMO_MESH_ISO = 30.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True)
    ap.add_argument("--make-demo")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--encoding", default="hash")
    ap.add_argument("--out", default="train_synthetic_view.png")
    ap.add_argument("--device-batches", action="store_true",
                    help="keep the frames on the device as uint8 (api.ImageSet) and draw every batch there (Trainer.step_images) "
                         "instead of gathering it from a per-ray dataset")
    ap.add_argument("--loss", default="l2", choices=sorted(api.LOSS_KINDS), help="the training loss (Trainer(loss=...))")
    ap.add_argument("--opacity-weight", type=float, default=0.0,
                    help="> 0: load the frames with their alpha (RGBA, trained over white) and fit the rays' opacity to it with this weight")
    ap.add_argument("--distortion-weight", type=float, default=0.0,
                    help="> 0: mip-NeRF 360's distortion regulariser with this weight, for world distances along the ray (a weight quoted "
                         "for distances normalised to [0, 1] is divided by 2 sqrt(3)); raise --loss-scale with it")
    ap.add_argument("--depth", action="store_true", help="--make-demo also writes analytic 16-bit depth PNGs of the teacher and their JSON keys")
    ap.add_argument("--depth-weight", type=float, default=0.0,
                    help="lambda_z of the depth term (Trainer(depth_weight=...), DESIGN 5.22): train with the scene's depth maps "
                         "(depth_file_path / depth_path in its transforms_train.json); batches are drawn on the device")
    ap.add_argument("--depth-loss", default="l2", choices=sorted(api.DEPTH_LOSS_KINDS), help="the depth term's loss")
    ap.add_argument("--loss-scale", default="128", metavar="S|dynamic",
                    help="the fp16 gradients' loss scale: the regulariser's gradient is largely rounded away at the default (DESIGN 5.12); "
                         "'dynamic': kept on the device, halved when a step's gradients are not finite and doubled after "
                         "--growth-interval clean steps (DESIGN 5.14)")
    ap.add_argument("--growth-interval", type=int, default=2000, help="--loss-scale dynamic: clean steps between two doublings")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="clip the total gradient norm to X (Trainer(max_grad_norm=...)); with a fixed --loss-scale that must be a power of two")
    ap.add_argument("--lr-schedule", default=None, metavar="nerf|instant_ngp|cosine:N",
                    help="decay the learning rates on the device (Trainer(lr_schedule=...)): NeRF's x0.1 per 250k steps, instant-ngp's x0.33 "
                         "every 10k steps after 20k, or a cosine to 0.01 of the rate over N steps")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="AdamW's decoupled weight decay on the MLP")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="skip a step whose gradients hold an Inf or a NaN instead of stepping Adam on them; the number skipped is printed")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="keep the debiased exponential moving average of the weights with this decay (Trainer(ema_decay=...), DESIGN 5.15) "
                         "and report the held-out PSNR and SSIM of the averaged weights (evaluate(weights='ema')) beside the live ones")
    ap.add_argument("--refine-poses", nargs="?", const=1e-3, type=float, default=None, metavar="LR",
                    help="refine a 6-DoF correction per training image on the device from the rays' gradients "
                         "(Trainer(ray_gradients=True), attach_images(refine_poses=...), DESIGN 5.16); implies --device-batches")
    ap.add_argument("--pose-noise", default=None, metavar="ROT_DEG,TRANS",
                    help="perturb the training poses on load by a seeded random rotation of ROT_DEG degrees and a translation of "
                         "length TRANS; the mean errors against the true poses are printed before and after training")
    ap.add_argument("--mesh", default=None, metavar="OUT.ply",
                    help="after training, extract the triangle mesh of {sigma * density_scale > iso} on the device "
                         "(Trainer.extract_mesh, DESIGN 5.19) and write it as a binary PLY, in the cube's coordinates")
    ap.add_argument("--mesh-resolution", type=int, default=128, metavar="N", help="lattice nodes per axis of --mesh")
    ap.add_argument("--mesh-iso", default=str(DEMO_MESH_ISO), metavar="V[,V...]",
                    help="iso value of --mesh, an extinction per unit length of the cube; the default is a judgement call from a sweep on "
                         "the --make-demo scene (DESIGN 5.19), not a derived number.  Several values: one OUT.<V>.ply each, and the sweep's table")
    ap.add_argument("--lens", default=None, metavar="MODEL:k1,k2,...",
                    help="--make-demo renders its frames through this lens (opencv: k1,k2,k3,p1,p2; opencv_fisheye: k1,k2,k3,k4) and writes "
                         "its intrinsics into transforms_train.json (DESIGN 5.20)")
    ap.add_argument("--assume-pinhole", action="store_true",
                    help="ignore the intrinsics in transforms_train.json and train and score under the centred pinhole of camera_angle_x")
    ap.add_argument("--intrinsics-noise", default=None, metavar="focal=F,center=C",
                    help="perturb the training cameras on load: fx and fy by a seeded factor exp(+-F), the principal point by C pixels in "
                         "a seeded direction; the errors against the file's cameras are printed before and after training")
    ap.add_argument("--refine-cameras", nargs="?", const="", default=None, metavar="focal=LR,center=LR,distortion=LR",
                    help="refine the cameras' intrinsics on the device beside the weights (attach_images(refine_cameras=...), DESIGN 5.21); "
                         "rates per group, 0 freezes one, defaults api.CAMERA_REFINE_DEFAULTS; needs a scene with cameras and --encoding hash")
    a = ap.parse_args()
    json_path = os.path.join(a.data, "transforms_train.json")
    if a.make_demo:
        torch.cuda.set_device(0)
        make_demo(a.make_demo, lens=parse_lens(a.lens) if a.lens else None, depth=a.depth)
    elif a.lens or a.depth:
        sys.exit("--lens / --depth describe the scene --make-demo writes; a loaded scene's cameras and depth maps come from its "
                 "transforms_train.json")
    # a scene whose JSON carries intrinsics (fl_x ...) is trained and scored with them: batches drawn on the device through the cameras
    with open(json_path) as f:
        top = json.load(f)
    use_cameras = not a.assume_pinhole and ("fl_x" in top or any("fl_x" in fr for fr in top.get("frames", [])))
    if use_cameras:
        a.device_batches = True
    if a.depth_weight > 0.0:
        a.device_batches = True            # the depth targets are formed on the device from the drawn pixels
    if a.refine_poses is not None:
        a.device_batches = True
        if a.encoding != "hash":
            sys.exit("--refine-poses needs --encoding hash (ray gradients go through the hash grid)")
    refine_cameras = None
    if a.refine_cameras is not None or a.intrinsics_noise:
        if not use_cameras:
            sys.exit("--refine-cameras / --intrinsics-noise need a scene whose transforms_train.json carries intrinsics (--make-demo --lens ...)")
    if a.refine_cameras is not None:
        if a.encoding != "hash":
            sys.exit("--refine-cameras needs --encoding hash (ray gradients go through the hash grid)")
        rates = parse_groups(a.refine_cameras, ("focal", "center", "distortion"), "--refine-cameras")
        refine_cameras = {f"lr_{k}": v for k, v in rates.items()} or True
    loss_scale = api.loss_scaler(growth_interval=a.growth_interval) if a.loss_scale == "dynamic" else float(a.loss_scale)
    schedule = a.lr_schedule
    if schedule and schedule.startswith("cosine:"):
        schedule = dict(kind="cosine", decay_steps=int(schedule.split(":", 1)[1]), ratio=0.01)
    torch.cuda.set_device(0)
    # flags=2: keep the PNGs' sRGB values (the reference's stbi_loadf applies a 2.2 gamma, Q11); corrected focal (Q1);
    # origin/10 as in the reference (Q2) so that Blender's radius-4 cameras sit just outside the unit grid
    rgba = a.opacity_weight > 0.0
    C = 4 if rgba else 3
    ds = loader.load_images_json(a.data, "train", flags=2 | (4 if rgba else 0))      # 4: RTXN_LOAD_RGBA
    if ds.images.shape[0] == 0:
        sys.exit("no frames loaded")
    if rgba and float(ds.images[..., 3].min()) == 1.0:
        sys.exit("--opacity-weight: these frames carry no alpha (every pixel is opaque): there is no mask to fit")
    n_hold = max(1, ds.images.shape[0] // 8)
    true_poses = np.array(ds.poses[:-n_hold], np.float32).reshape(-1, 4, 4)
    train_poses = true_poses
    if a.pose_noise:
        rot_deg, trans = (float(v) for v in a.pose_noise.split(","))
        train_poses = perturb_poses(true_poses, rot_deg, trans, seed=0)
    cams_train = cams_hold = None
    if use_cameras:
        model, P = loader.read_cameras(json_path, ds.image_width, ds.image_height)
        true_P = P[:1] if P.shape[0] == 1 else P[:-n_hold]
        if a.intrinsics_noise:
            noise = parse_groups(a.intrinsics_noise, ("focal", "center"), "--intrinsics-noise")
            P = perturb_cameras(P, noise.get("focal", 0.0), noise.get("center", 0.0))
        loaded_P = (P[:1] if P.shape[0] == 1 else P[:-n_hold]).copy()
        if P.shape[0] == 1:
            cams_train = cams_hold = api.camera_set(model, P, width=ds.image_width, height=ds.image_height)
        else:                  # one camera per frame: the held-out frames are the last n_hold
            cams_train = api.camera_set(model, P[:-n_hold], width=ds.image_width, height=ds.image_height)
            cams_hold = api.camera_set(model, P[-n_hold:], width=ds.image_width, height=ds.image_height)
        print(f"cameras: {model}, {P.shape[0]} in {json_path}" + ("" if P.shape[0] > 1 else " (shared by every frame)"))
    train_ds = loader.ImageDataset(ds.images[:-n_hold], train_poses.reshape(ds.poses[:-n_hold].shape), ds.focal, ds.image_width, ds.image_height, C, ds.camera_angle_x)
    if a.device_batches:
        # flags=2 frames are k/255: one byte per channel holds them exactly
        depth_kw = {}
        if a.depth_weight > 0.0:
            maps, unit = loader.read_depth_maps(json_path, ds.image_width, ds.image_height)
            depth_kw = dict(depth=maps[:-n_hold], depth_unit=unit, depth_kind="z")
            print(f"depth maps: {maps.dtype} in units of {unit:g}, {100.0 * float((maps[:-n_hold] > 0).mean()):.1f}% of the training pixels "
                  f"carry a value")
        images, focal = api.ImageSet.from_dataset(train_ds, storage="u8", cameras=cams_train, **depth_kw)
        n_rays, held = images.n_images * images.width * images.height, images.nbytes()
    else:
        rays, focal = RayDataset.from_images(train_ds, origin_scale=0.1)
        n_rays, held = rays.n, sum(t.numel() * t.element_size() for t in (rays.rays_o, rays.rays_d, rays.pixels))
    R = a.grid
    model = dict(encoding=a.encoding, n_neurons=64, n_hidden_layers=2 if a.encoding == "hash" else 4,
                 hashgrid=dict(n_levels=8, n_features=2, log2_hashmap_size=15, base_resolution=8, per_level_scale=1.5),
                 batch_rays=max(a.batch, ds.image_width * ds.image_height), max_segments=max(a.batch, ds.image_width * ds.image_height) * (3 * R),
                 density_scale=150.0)
    tr = Trainer(R, None, lr=1e-2 if a.encoding == "hash" else 2e-3, loss=a.loss, opacity_weight=a.opacity_weight,
                 background=(1.0, 1.0, 1.0) if rgba else None, target_channels=C, distortion_weight=a.distortion_weight,
                 loss_scale=loss_scale, lr_schedule=schedule, weight_decay=a.weight_decay, skip_nonfinite=a.skip_nonfinite,
                 max_grad_norm=a.max_grad_norm, ema_decay=a.ema_decay, depth_weight=a.depth_weight, depth_loss=a.depth_loss,
                 ray_gradients=a.refine_poses is not None or refine_cameras is not None, **model)
    white = (1.0, 1.0, 1.0) if rgba else None
    # the held-out frames stay on the device as they were loaded (flags=2 frames are k/255: one byte per channel holds them exactly)
    hold_ds = loader.ImageDataset(ds.images[-n_hold:], ds.poses[-n_hold:], ds.focal, ds.image_width, ds.image_height, C, ds.camera_angle_x)
    hold, _ = api.ImageSet.from_dataset(hold_ds, storage="u8", cameras=cams_hold)

    def render():
        return tr.render_rays(o_t, d_t, background=white)

    def score(weights="live"):
        """mean PSNR and SSIM over ALL held-out frames (Trainer.evaluate: rendered and compared on the device, an RGBA frame over
        the white the model is trained over); one host read, of the two means"""
        _, db, ssim = tr.evaluate(hold, weights=weights).mean(0).tolist()
        return f"{db:.2f} dB, SSIM {ssim:.4f}"

    def held_out():
        return score() if a.ema_decay is None else f"{score()} live, {score('ema')} averaged"

    if a.device_batches:
        tr.attach_images(images, refine_poses=None if a.refine_poses is None else dict(lr=a.refine_poses), refine_cameras=refine_cameras)
    g = torch.Generator(device="cuda").manual_seed(0)
    W, H = ds.image_width, ds.image_height
    if use_cameras:
        o_t, d_t = api.camera_rays(cams_hold, cams_hold.n_cameras - 1, hold.poses[-1], W, H)
    else:
        o_t, d_t = camera_rays(ds.poses[-1], focal, W, H, origin_scale=0.1)
    print(f"{n_rays} training rays from {train_ds.images.shape[0]} frames ({W}x{H}), {held / 1e6:.2f} MB on the device "
          f"({'image set, batches drawn on the device' if a.device_batches else 'ray dataset'}); held-out PSNR over {n_hold} frame{'s' if n_hold > 1 else ''} before: {held_out()}")
    for it in range(a.steps):
        loss = tr.step_images(a.batch) if a.device_batches else tr.step(*rays.sample_batch(a.batch, g))
        if (it + 1) % 100 == 0:
            frac = tr.update_occupancy(threshold=0.01) if it + 1 >= 200 else 1.0
            print(f"step {it + 1:5d} loss {float(loss.item()):.6f} lr {tr.current_lr():.3e} occupied {100 * frac:.1f}% held-out PSNR "
                  f"{held_out()}", flush=True)
    print(f"final held-out PSNR after {a.steps} steps ({'device batches' if a.device_batches else 'ray dataset'}): "
          f"{held_out()}")
    if a.pose_noise or a.refine_poses is not None:
        r0, t0 = pose_errors(train_poses, true_poses)
        line = f"training poses against the true ones: mean rotation error {r0:.4f} deg, mean translation error {t0:.5f} as loaded"
        if a.refine_poses is not None:
            r1, t1 = pose_errors(tr.refined_poses().cpu().numpy(), true_poses)
            line += f"; {r1:.4f} deg, {t1:.5f} after refinement ({int(tr.pose_updates.min().item())}+ updates per image)"
        print(line)
    if use_cameras and (a.intrinsics_noise or refine_cameras is not None):
        # a camera shared by every frame is shared with the held-out set too: the scores above are under the refined row
        f0, c0 = camera_errors(loaded_P, true_P)
        line = f"training cameras against the file's: mean |log focal ratio| {f0:.5f}, mean principal-point error {c0:.3f} px as loaded"
        if refine_cameras is not None:
            tr.check_cameras()                 # the live rows are still invertible over the frame (raises naming camera and pixel)
            refined = tr.refined_cameras().cpu().numpy()
            f1, c1 = camera_errors(refined, true_P)
            line += f"; {f1:.5f}, {c1:.3f} px after refinement ({int(tr.camera_updates.min().item())}+ updates per camera)"
        print(line)
        np.set_printoptions(precision=5, suppress=True, linewidth=200)
        print("rows (fx fy cx cy k1 k2 k3 k4 p1 p2), camera 0:\n  loaded ", loaded_P[0, :10])
        if refine_cameras is not None:
            print("  refined", refined[0, :10])
        print("  true   ", np.asarray(true_P)[0, :10])
    if tr.loss_scale_now is not None:
        print(f"loss scale now {float(tr.loss_scale_now.item()):g}: {int(tr.skipped_steps.item())} steps skipped, "
              f"{int(tr.scale_backoffs.item())} backoffs, {int(tr.scale_growths.item())} growths, {int(tr.clipped_steps.item())} steps clipped, "
              f"last gradient norm {float(tr.grad_norm.item()):.3e}")
    elif tr.skipped_steps is not None and a.skip_nonfinite:
        print(f"steps skipped for non-finite gradients: {int(tr.skipped_steps.item())} (many: lower --loss-scale, or --loss-scale dynamic)")
    img = render().reshape(H, W, 3).cpu().numpy()
    loader.write_png(a.out, img)
    print("wrote", a.out)
    if a.mesh:
        isos = [float(v) for v in a.mesh_iso.split(",")]
        for iso in isos:
            v, t, nrm = tr.extract_mesh(a.mesh_resolution, iso=iso, weights="live" if a.ema_decay is None else "ema")
            path = a.mesh if len(isos) == 1 else f"{os.path.splitext(a.mesh)[0]}.{iso:g}.ply"
            api.write_ply(path, v, t, nrm)
            # closed: every undirected edge belongs to two triangles (an open one ends on a face of the cube)
            e = torch.sort(torch.cat([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).long(), dim=1).values
            _, per_edge = torch.unique(e[:, 0] * max(v.shape[0], 1) + e[:, 1], return_counts=True)
            closed = bool((per_edge == 2).all().item())
            print(f"mesh at iso {iso:g}, {a.mesh_resolution}^3 nodes: {v.shape[0]} vertices, {t.shape[0]} triangles, "
                  f"{'closed' if closed else 'open'}; wrote {path}")


if __name__ == "__main__":
    main()
