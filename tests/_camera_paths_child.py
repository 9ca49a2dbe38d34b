"""Child process of tests/test_gpu_camera.py (run with RTXN_DETERMINISTIC=1 in the environment, so every Trainer made here is
deterministic): the tiny hash model of test_gpu_draw_batch.py, 256 rays, 3 steps on a 3-frame image set WITH cameras, through
step_images, capture_step(draw=True) with and without prefetch, entry_args(draw=True) / step_entry, and a trainer without a set
fed the same batches by hand (api.draw_batch with the set's cameras, then step()).  Prints one JSON line: per path the SHA-256 of
the parameters after every step, the by-hand path once more without cameras, and the drawn (image, pixel) of the last batch."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

R, B, STEPS = 16, 256, 3
N_IMG, W, H = 3, 40, 30
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)


def main():
    import torch
    import _camera_float64 as F
    from rtx_nerf_amd import api, scenes
    from rtx_nerf_amd.train import Trainer
    assert os.environ.get("RTXN_DETERMINISTIC") == "1"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(11)
    frames = torch.from_numpy(rng.integers(0, 256, (N_IMG, H, W, 3), dtype=np.uint8)).cuda()
    poses = torch.from_numpy(np.stack([np.asarray(scenes.pose_spherical(35.0 + 110.0 * i, -25.0 - 10.0 * i, origin_scale=10.0), np.float32).reshape(16)
                                       for i in range(N_IMG)])).cuda()
    rows = np.stack([F.opencv_params(F.OPENCV_SETS[i + 1], fx=F.FX + i, cy=F.CY - i) for i in range(N_IMG)])
    cams = api.camera_set("opencv", rows, width=W, height=H)
    focal = 2.0 * float(F.FX) / H                              # the centred pinhole nearest to the cameras: what "no cameras" means
    with_cams = api.ImageSet(frames, poses, cameras=cams)
    without = api.ImageSet(frames, poses, focal)
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()

    def trainer(iset=None):
        tr = Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=4, hashgrid=HGD, n_dir_freqs=4, batch_rays=B, max_segments=B * 30,
                     lr=1e-2, loss_scale=128.0, density_scale=120.0, mode="nerf", seed=3, sample_jitter=True, jitter_seed=21)
        assert tr.deterministic
        if iset is not None:
            tr.attach_images(iset)
        return tr

    def digest(tr):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (tr.params, tr.master, tr.table, tr.table_master):
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        return h.hexdigest()

    out = {}

    def by_hand(iset):
        tr, got = trainer(), []
        o, d, t = torch.empty((B, 3), device="cuda"), torch.empty((B, 3), device="cuda"), torch.empty((B, 3), device="cuda")
        dr = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        for k in range(STEPS):
            api.draw_batch(iset, B, 0, torch.full((1,), k, dtype=torch.int32, device="cuda"), o, d, t, dr)
            tr.step(o, d, t)
            assert int(tr.total.item()) > B                   # the batch crosses the occupied sphere
            got.append(digest(tr))
        return got, dr.cpu().numpy().tolist()

    out["by_hand"], out["drawn"] = by_hand(with_cams)
    out["by_hand_without_cameras"], drawn_plain = by_hand(without)
    assert drawn_plain == out["drawn"]                        # the same (image, pixel): only the rays differ

    tr = trainer(with_cams)
    out["step_images"] = []
    for _ in range(STEPS):
        tr.step_images()
        out["step_images"].append(digest(tr))
    assert tr.drawn[:B].cpu().numpy().tolist() == out["drawn"]

    for prefetch in (False, True):
        tr = trainer(with_cams)
        tr.capture_step(B, launch_segments=B * 30, prefetch=prefetch, draw=True)
        got = []
        if prefetch:
            assert tr.step_captured() is None
        for k in range(STEPS):
            tr.step_captured() if (not prefetch or k < STEPS - 1) else tr.flush_captured()
            got.append(digest(tr))
        out["captured_prefetch" if prefetch else "captured"] = got

    tr = trainer(with_cams)
    args, dargs = tr.entry_args(B, launch_segments=B * 30, draw=True)
    assert dargs._cameras is cams
    out["step_entry"] = []
    for _ in range(STEPS):
        tr.step_entry()
        out["step_entry"].append(digest(tr))
    print("CAMERA_PATHS " + json.dumps(out))


if __name__ == "__main__":
    main()
