"""Intrinsics refinement on the GPU against the float64 restatement of tests/_intrinsics_float64.py, which
tests/test_intrinsics_float64_reference.py holds to central differences.
  * the gradient (rtxn_camera_gradients) over the 40 x 30 frame and the eight lens cases of tests/_camera_float64.py, 1, 255, 257
    and 1025 rays, a shared camera and three per-image cameras of which one is never drawn, a fisheye camera whose principal point
    is a pixel centre; the count, the zero rows and entries, two calls and two paddings bit-identical;
  * the step (rtxn_camera_step): 50 steps of the float64 recurrence re-seeded from the device's own state with cameras dropping in
    and out, the clamp, a frozen group, delta == 0, a NaN gradient, the skip word, and the rays the next draw generates;
  * the Trainer: the direct calls, the three stepping paths bit-identical, None and rate 0 bit-identical to a run without the
    argument, beside refine_poses, a checkpoint, check_cameras() and the refusals.

THE GRADIENT'S BOUND.  |got - want| <= C 2^-24 S per camera and parameter, S = sum_r |term_r| in float64.  C cannot be derived:
the error of the fp32 Newton solution enters every term through J^-1 (1 / dpoly), by an amount that depends on the lens.  It was
measured against the float64 restatement over every case below -- the worst err / (2^-24 S) was 2.06 for the pinhole, 6.58 for
OPENCV and 9.48 for OPENCV_FISHEYE, each at a single ray, where nothing averages -- and C is four times the worst of them, rounded
up to a power of two: 4 x 9.48 = 37.9 -> 64.  The seeded defect (the k2 term 3 % off) misses it by more than an order of magnitude."""
import faulthandler

import numpy as np
import pytest

import _camera_float64 as F
import _intrinsics_float64 as I
import _ray_gradient_float64 as G

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_BOUND = 64.0
BAR_D = 2e-6              # generated ray directions against float64, per component: tests/test_gpu_camera.py's bar
W, H = F.W, F.H
CASES = F.all_cases()
SENT = -7.75


@pytest.fixture(autouse=True)
def _own_timeout():
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poses(n):
    from rtx_nerf_amd import scenes
    return np.stack([np.asarray(scenes.pose_spherical(35.0 + 80.0 * i, -25.0 - 10.0 * i, origin_scale=10.0), np.float32).reshape(16)
                     for i in range(n)])


CFG = dict(lr_focal=1e-3, lr_center=1e-2, lr_distortion=1e-4, max_log_focal=0.06, max_center=2.0, max_distortion=0.01, beta1=0.9,
           beta2=0.999, eps=1e-15)


def _state(torch, api, model, rows, n_rays=1, skip=None, cfg=CFG, st=None):
    rows = np.asarray(rows, np.float32).reshape(-1, 12)
    K = len(rows)
    if st is None:
        st = dict(params0=_dev(torch, rows), params=_dev(torch, rows).clone(), delta=torch.zeros((K, 10), device="cuda"),
                  m=torch.zeros((K, 10), device="cuda"), v=torch.zeros((K, 10), device="cuda"),
                  steps=torch.zeros(K, dtype=torch.int32, device="cuda"), grad=torch.zeros((K, 12), device="cuda"),
                  terms=torch.zeros((n_rays, 12), device="cuda"), skipped=torch.zeros(1, dtype=torch.int32, device="cuda"))
    return st, api.camera_refinement(model, K, W, **cfg, skip=skip, **st)


# ------------------------------------------------------------------------------------------------ the gradient
def _layout(name, model, row, layout):
    """(camera rows, n_images): shared = the case's row for three images; per_image = three cameras, the third never drawn;
    principal = the fisheye whose principal point is the centre of pixel (18, 16), shared"""
    if layout == "shared":
        return row[None], 3
    if layout == "principal":
        return F.fisheye_params(tuple(row[4:8]), cx=18.5, cy=16.5)[None], 3
    second = row.copy()
    second[:4] = (29.0, 33.5, 21.25, 13.75)
    if model == F.OPENCV_FISHEYE:
        second[2:4] = (18.5, 16.5)
    return np.stack([row, second, row]), 3


def _inputs(model, rows, n_rays, seed):
    rng = np.random.default_rng(seed)
    drawn = np.stack([rng.integers(0, 2, n_rays), rng.integers(0, W * H, n_rays)], 1).astype(np.int32)      # image 2 is never drawn
    if model == F.OPENCV_FISHEYE and n_rays > 1:
        drawn[n_rays // 2] = (1, 16 * W + 18)                # thd < 1e-8 under a camera with (cx, cy) = (18.5, 16.5)
    g = (rng.standard_normal((n_rays, 3)) * 1e-5).astype(np.float32)
    return drawn, g


LAYOUTS = [(c, lay) for c in CASES for lay in ("shared", "per_image")] + [(c, "principal") for c in CASES if c[1] == F.OPENCV_FISHEYE]
_worst = {}


@pytest.mark.parametrize("case,layout", LAYOUTS, ids=[f"{c[0]}-{lay}" for c, lay in LAYOUTS])
def test_camera_gradient_matches_float64(gpu, case, layout):
    torch = gpu
    from rtx_nerf_amd import api
    name, model, row = case
    rows, n_images = _layout(name, model, row, layout)
    poses = _poses(n_images)
    K = len(rows)
    for n_rays in (1, 255, 257, 1025):
        drawn, g = _inputs(model, rows, n_rays, 7 * n_rays + len(name))
        st, cams = _state(torch, api, model, rows, n_rays)
        st["grad"].fill_(SENT)
        args = (_dev(torch, drawn), _dev(torch, g), n_rays, _dev(torch, poses))
        api.camera_gradients(*args, cams)
        got = st["grad"].cpu().numpy()
        want, S = I.camera_gradients(model, rows, poses, drawn, W, g)
        assert np.array_equal(got[:, 10], want[:, 10]) and np.all(got[:, 11] == 0), (n_rays, got[:, 10:])           # the count, the pad
        if K > 1:
            assert got[2].tobytes() == np.zeros(12, np.float32).tobytes()                                          # never drawn
        absent = [e for e in range(10) if e not in I.HAS[model]]
        assert np.all(got[:, absent] == 0) and not np.signbit(got[:, absent]).any()
        assert np.isfinite(got).all()
        err = np.abs(got[:, :10].astype(np.float64) - want[:, :10])
        ratio = float((err / np.where(S > 0, U * S, 1.0)).max())
        _worst[model] = max(_worst.get(model, 0.0), ratio)
        print(f"measured {name} {layout} n_rays={n_rays}: worst err / (2^-24 sum|terms|) = {ratio:.3f} (model so far {_worst[model]:.3f})")
        assert np.all(err <= C_BOUND * U * S), (n_rays, ratio)
        if model == F.OPENCV_FISHEYE and n_rays > 1 and (layout == "principal" or K > 1):
            t = st["terms"][n_rays // 2].cpu().numpy()                                                              # the pinhole branch
            assert np.all(t[4:] == 0) and np.all(t[:2] == 0) and np.all(t[2:4] != 0)             # xd = yd = 0: no focal term either
        # a second call: the same bytes; the same rays in a larger launch behind other rays' scratch: the same bytes
        first = st["grad"].clone()
        api.camera_gradients(*args, cams)
        assert torch.equal(first, st["grad"])
        pad = 300
        st2, cams2 = _state(torch, api, model, rows, n_rays + pad)
        st2["terms"].fill_(float("nan"))
        big_d, big_g = np.zeros((n_rays + pad, 2), np.int32), np.full((n_rays + pad, 3), np.nan, np.float32)
        big_d[:n_rays], big_g[:n_rays] = drawn, g
        api.camera_gradients(_dev(torch, big_d), _dev(torch, big_g), n_rays, args[3], cams2)
        assert torch.equal(first, st2["grad"]) and bool(torch.isnan(st2["terms"][n_rays:]).all())                   # nothing past n_rays
        if n_rays == 1025 and model != F.PINHOLE:
            # the negative control: a k2 term 3 % off misses the same bound
            bad, _ = I.camera_gradients(model, rows, poses, drawn, W, g, scale_k2=1.03)
            assert np.any(np.abs(got[:, 5] - bad[:, 5]) > C_BOUND * U * S[:, 5])


# ------------------------------------------------------------------------------------------------ the step
NAMES = ("delta", "m", "v", "steps", "params")


def _snap(st):
    return {k: st[k].cpu().numpy() for k in NAMES}


@pytest.mark.parametrize("model", [F.OPENCV, F.OPENCV_FISHEYE, F.PINHOLE], ids=["opencv", "fisheye", "pinhole"])
def test_camera_step_follows_the_float64_recurrence(gpu, model):
    torch = gpu
    from rtx_nerf_amd import api
    K = 4
    base = {F.OPENCV: F.opencv_params(F.OPENCV_SETS[1]), F.OPENCV_FISHEYE: F.fisheye_params(F.FISHEYE_SETS[1]), F.PINHOLE: F.params()}[model]
    rows0 = np.stack([base] * K)
    rows0[:, :4] += np.arange(K, dtype=np.float32)[:, None] * 0.25
    rows0[1, 10] = -0.0                                   # a signed zero in a pad word survives
    rows0[2, 7 if model == F.OPENCV else 9] = 0.125       # an entry the model lacks keeps whatever it was loaded with
    st, cams = _state(torch, api, model, rows0)
    st["params"].fill_(SENT)
    api.camera_compose(cams)
    assert st["params"].cpu().numpy().tobytes() == rows0.tobytes()          # delta == 0: params0 bit for bit
    rng = np.random.default_rng(50 + model)
    worst = dict(delta=0.0, m=0.0, v=0.0, params=0.0)
    has = I.HAS[model]
    absent = [e for e in range(10) if e not in has]
    for step in range(50):
        grad = np.zeros((K, 12), np.float32)
        grad[:, :10] = rng.standard_normal((K, 10)) * 10.0 ** rng.uniform(-8, -4, (K, 1))
        grad[:, 10] = rng.integers(0, 3, K) * (rng.random(K) < 0.7)          # cameras drop in and out of the batch
        grad[0, 10] = 5 if step % 2 == 0 else 0
        st["grad"].copy_(_dev(torch, grad))
        before = _snap(st)
        api.camera_step(cams)
        after = _snap(st)
        for i in range(K):
            if grad[i, 10] == 0:
                assert all(before[k][i].tobytes() == after[k][i].tobytes() for k in NAMES), (step, i)
                continue
            d1, m1, v1, t, b_d, b_m, b_v, active = I.camera_step(model, CFG, before["params"][i], before["delta"][i], before["m"][i],
                                                                 before["v"][i], before["steps"][i], grad[i])
            assert after["steps"][i] == t and active == has
            for k, want, b in (("delta", d1, b_d), ("m", m1, b_m), ("v", v1, b_v)):
                ratio, bad = G.check(after[k][i], want, b)
                worst[k] = max(worst[k], ratio)
                assert bad == 0, (step, i, k, ratio)
                assert after[k][i][absent].tobytes() == before[k][i][absent].tobytes()
            want, b = I.compose_row(model, rows0[i], after["delta"][i])
            ratio, bad = G.check(after["params"][i], want, b)
            worst["params"] = max(worst["params"], ratio)
            assert bad == 0, (step, i, "params", ratio)
            assert after["params"][i][absent + [10, 11]].tobytes() == rows0[i][absent + [10, 11]].tobytes()
    print("measured camera step, worst err / bound over 50 steps: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    delta = st["delta"].cpu().numpy()
    assert int(st["steps"].max()) > 10 and np.abs(delta[:, :2]).max() > 1e-3 and int(st["skipped"].item()) == 0
    assert np.all(np.abs(delta[:, :2]) <= np.float32(CFG["max_log_focal"])) and np.all(delta[:, absent] == 0)

    # the next draw generates the float64 rays of the refined rows
    poses = _poses(K)
    cset = api.CameraSet(model, st["params"])
    iset = api.ImageSet(torch.zeros((K, H, W, 3), device="cuda"), _dev(torch, poses), cameras=cset)
    n = 512
    o, d, tg = (torch.zeros((n, 3), device="cuda") for _ in range(3))
    dr = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    api.draw_batch(iset, n, 3, None, o, d, tg, dr)
    d, dr = d.cpu().numpy().astype(np.float64), dr.cpu().numpy()
    for i in range(K):
        row64, _ = I.compose_row(model, rows0[i], delta[i])
        _, want = F.camera_rays(model, row64, poses[i], W, H)
        sel = dr[:, 0] == i
        assert sel.any() and np.abs(d[sel] - want[dr[sel, 1]]).max() <= BAR_D, (i, np.abs(d[sel] - want[dr[sel, 1]]).max())

    # a rate-0 group keeps every bit while the others move
    frozen = dict(CFG, lr_center=0.0)
    _, cams_f = _state(torch, api, model, rows0, cfg=frozen, st=st)
    grad = np.zeros((K, 12), np.float32)
    grad[:, :10], grad[:, 10] = 1e-6, 2
    st["grad"].copy_(_dev(torch, grad))
    before = _snap(st)
    api.camera_step(cams_f)
    after = _snap(st)
    for k in ("delta", "m", "v", "params"):
        assert after[k][:, 2:4].tobytes() == before[k][:, 2:4].tobytes(), k
        assert not np.array_equal(after[k][:, :2], before[k][:, :2]), k
    assert np.all(after["steps"] == before["steps"] + 1)
    # every group frozen: nothing moves, not even the count
    _, cams_0 = _state(torch, api, model, rows0, cfg=dict(CFG, lr_focal=0.0, lr_center=0.0, lr_distortion=0.0), st=st)
    before = _snap(st)
    api.camera_step(cams_0)
    assert all(before[k].tobytes() == v.tobytes() for k, v in _snap(st).items())

    # a rate large enough that delta meets its clamp, and stays there
    hot = dict(CFG, lr_center=1.5, max_center=2.0)
    _, cams_h = _state(torch, api, model, rows0, cfg=hot, st=st)
    grad[:, 2:4] = 1e-2                                   # large beside the moments the 50 steps left
    st["grad"].copy_(_dev(torch, grad))
    for _ in range(8):
        api.camera_step(cams_h)
    after = _snap(st)
    assert np.all(after["delta"][:, 2:4] == -2.0), after["delta"][:, 2:4]
    assert np.array_equal(after["params"][:, 2:4], rows0[:, 2:4] + np.float32(-2.0))
    assert np.all(np.abs(after["delta"][:, :2]) <= np.float32(CFG["max_log_focal"]))

    # a non-finite gradient: that camera keeps every word and the count goes up; the others step
    grad[1, 3] = np.nan
    st["grad"].copy_(_dev(torch, grad))
    before = _snap(st)
    api.camera_step(cams)
    after = _snap(st)
    assert all(before[k][1].tobytes() == after[k][1].tobytes() for k in NAMES) and int(st["skipped"].item()) == 1
    assert after["steps"][0] == before["steps"][0] + 1 and after["delta"][0].tobytes() != before["delta"][0].tobytes()
    if absent:                                            # ... but a NaN in an entry the model lacks is not looked at
        grad[1, 3], grad[1, absent[0]] = 1e-6, np.nan
        st["grad"].copy_(_dev(torch, grad))
        api.camera_step(cams)
        assert int(st["skipped"].item()) == 1 and st["steps"].cpu().numpy()[1] == after["steps"][1] + 1
    # the guard's skip word: nothing moves for any camera, and nothing is counted
    grad[1, :10] = 1e-6
    st["grad"].copy_(_dev(torch, grad))
    skip = torch.ones(1, dtype=torch.int32, device="cuda")
    _, guarded = _state(torch, api, model, rows0, skip=skip, st=st)
    before = _snap(st)
    api.camera_step(guarded)
    assert all(before[k].tobytes() == v.tobytes() for k, v in _snap(st).items()) and int(st["skipped"].item()) == 1


# ------------------------------------------------------------------------------------------------ the Trainer
R, B, N_IMG, TW, TH = 16, 256, 4, 16, 12
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
RATES = dict(lr_focal=1e-3, lr_center=1e-2, lr_distortion=1e-4)
FROZEN = dict(lr_focal=0.0, lr_center=0.0, lr_distortion=0.0)


def _rows(n):
    k = F.OPENCV_SETS[0]
    return np.stack([F.opencv_params(k, fx=14.0 + 0.5 * i, fy=13.5 - 0.25 * i, cx=8.2 + 0.1 * i, cy=5.9 - 0.1 * i) for i in range(n)])


def _image_set(torch, n_cameras=N_IMG, cameras=True):
    """a fresh set every time: the refinement rewrites its rows (and poses) in place"""
    from rtx_nerf_amd import api, scenes
    img = np.random.default_rng(103).uniform(0, 1, (N_IMG, TH, TW, 3)).astype(np.float32)
    cams = api.camera_set("opencv", _rows(n_cameras), TW, TH) if cameras else None
    return api.ImageSet(torch.from_numpy(img).cuda(), torch.from_numpy(_poses(N_IMG)).cuda(), scenes.lego_focal_length(True), cameras=cams)


def _trainer(torch, refine_cameras=None, refine_poses=None, n_cameras=N_IMG, with_argument=True, **kw):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()
    args = dict(lr=1e-2, loss_scale=128.0, density_scale=120.0, mode="nerf", seed=3, deterministic=True, ray_gradients=True)
    args.update(kw)
    tr = Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=2, hashgrid=HGD, n_dir_freqs=4, batch_rays=B, max_segments=B * 30, **args)
    extra = dict(refine_cameras=refine_cameras) if with_argument else {}
    tr.attach_images(_image_set(torch, n_cameras), refine_poses=refine_poses, **extra)
    return tr


def _run(tr, path, steps=5):
    if path == "captured":
        tr.capture_step(B, launch_segments=B * 30, draw=True)
    elif path == "entry":
        tr.entry_args(B, launch_segments=B * 30, draw=True)
    fn = {"images": tr.step_images, "captured": tr.step_captured, "entry": tr.step_entry}[path]
    return [float(fn().item()) for _ in range(steps)]


def _tstate(tr):
    out = dict(params=tr.params, master=tr.master, table=tr.table, table_master=tr.table_master, poses=tr.image_set.poses,
               rows=tr.image_set.cameras.params, rays_d_grad=tr.rays_d_grad)
    if tr._cams is not None:
        out.update(camera_delta=tr.camera_delta, camera_updates=tr.camera_updates, camera_m=tr._cam_m, camera_v=tr._cam_v)
    if tr._pose is not None:
        out.update(pose_delta=tr.pose_delta, pose_updates=tr.pose_updates)
    return {k: v.clone() for k, v in out.items()}


def _assert_same(torch, a, b, what, keys=None):
    for k in (keys or a.keys()):
        assert torch.equal(a[k], b[k]), f"{what}: {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} differ"


@pytest.mark.parametrize("n_cameras", [1, N_IMG], ids=["shared", "per_image"])
def test_trainer_camera_gradient_equals_the_direct_calls(gpu, n_cameras):
    torch = gpu
    from rtx_nerf_amd import api
    tr = _trainer(torch, refine_cameras=FROZEN, n_cameras=n_cameras, sample_jitter=True, jitter_seed=21)
    tr.step_images()
    rows = tr.refined_cameras()
    assert torch.equal(rows, tr.cameras0) and int(tr.camera_updates.max()) == 0                # frozen: the rows are the draw's
    st, mine = _state(torch, api, F.OPENCV, rows.cpu().numpy(), B, cfg=dict(CFG, **FROZEN))
    mine.width = TW
    st["grad"].fill_(SENT)
    api.camera_gradients(tr.drawn, tr.rays_d_grad, B, tr.image_set.poses, mine)
    assert torch.equal(st["grad"], tr._cam_grad)
    got = st["grad"].cpu().numpy()
    assert got[:, 10].sum() == B and np.isfinite(got).all() and np.all(np.abs(got[:, [0, 1, 2, 3, 4, 8, 9]]).max(0) > 0) and np.all(got[:, 7] == 0)
    want, S = I.camera_gradients(F.OPENCV, rows.cpu().numpy(), tr.image_set.poses.cpu().numpy(), tr.drawn.cpu().numpy(), TW,
                                 tr.rays_d_grad.cpu().numpy())
    assert np.all(np.abs(got[:, :10] - want[:, :10]) <= C_BOUND * U * S)


@pytest.mark.parametrize("n_cameras", [1, N_IMG], ids=["shared", "per_image"])
def test_three_stepping_paths_refine_the_same_cameras(gpu, n_cameras):
    torch = gpu
    got = {}
    for path in ("images", "captured", "entry"):
        tr = _trainer(torch, refine_cameras=RATES, n_cameras=n_cameras, sample_jitter=True, jitter_seed=21)
        if path == "captured":
            rows_before = tr.image_set.cameras.params.clone()
            tr.capture_step(B, launch_segments=B * 30, draw=True)
            assert torch.equal(tr.image_set.cameras.params, rows_before) and int(tr.camera_updates.max()) == 0      # the warm-up is no step
            losses = [float(tr.step_captured().item()) for _ in range(5)]
        else:
            losses = _run(tr, path)
        got[path] = (_tstate(tr), losses)
        assert int(tr.camera_updates.min()) >= 4 and float(tr.camera_delta.abs().max()) > 1e-3 and int(tr.camera_skipped.item()) == 0
        assert float(tr.camera_delta[:, 7].abs().max()) == 0 and torch.equal(tr.refined_cameras()[:, [7, 10, 11]], tr.cameras0[:, [7, 10, 11]])
        assert not torch.equal(tr.refined_cameras()[:, :4], tr.cameras0[:, :4])
        tr.check_cameras()
    for path in ("captured", "entry"):
        _assert_same(torch, got["images"][0], got[path][0], path)
        assert got["images"][1] == got[path][1], path
    tr.reset_cameras()
    assert torch.equal(tr.image_set.cameras.params, tr.cameras0) and int(tr.camera_updates.max()) == 0
    assert float(tr.camera_delta.abs().max()) == 0


def test_none_and_zero_rates_leave_the_run_bit_identical(gpu):
    torch = gpu
    keys = ("params", "master", "table", "table_master", "poses", "rows", "rays_d_grad")
    plain = _trainer(torch, with_argument=False)
    want_losses = _run(plain, "images")
    want = _tstate(plain)
    for path in ("images", "captured", "entry"):
        for refine in (None, FROZEN):
            tr = _trainer(torch, refine_cameras=refine)
            assert (tr._cams is None) == (refine is None)
            if refine is None:
                assert not hasattr(tr, "camera_delta") and not hasattr(tr, "_cam_terms")                          # nothing allocated
            losses = _run(tr, path)
            _assert_same(torch, want, _tstate(tr), f"{path}, refine_cameras={refine}", keys)
            assert losses == want_losses, (path, refine)
            if refine is not None:
                assert float(tr.camera_delta.abs().max()) == 0 and int(tr.camera_updates.max()) == 0


def test_cameras_and_poses_refine_together_the_same_on_three_paths(gpu):
    torch = gpu
    got = {}
    for path in ("images", "captured", "entry"):
        tr = _trainer(torch, refine_cameras=RATES, refine_poses=dict(lr=1e-3), sample_jitter=True, jitter_seed=21)
        losses = _run(tr, path)
        got[path] = (_tstate(tr), losses)
        assert float(tr.camera_delta.abs().max()) > 1e-3 and float(tr.pose_delta.abs().max()) > 1e-3
        assert int(tr.camera_updates.min()) >= 4 and int(tr.pose_updates.min()) >= 4
        assert not torch.equal(tr.image_set.poses, tr.poses0) and not torch.equal(tr.image_set.cameras.params, tr.cameras0)
    for path in ("captured", "entry"):
        _assert_same(torch, got["images"][0], got[path][0], path)
        assert got["images"][1] == got[path][1], path
    # the poses alone move otherwise: the camera gradient reads, and the pose step is the one it was
    alone = _trainer(torch, refine_poses=dict(lr=1e-3), sample_jitter=True, jitter_seed=21)
    _run(alone, "images", steps=1)
    both = _trainer(torch, refine_cameras=RATES, refine_poses=dict(lr=1e-3), sample_jitter=True, jitter_seed=21)
    _run(both, "images", steps=1)
    assert torch.equal(alone.pose_delta, both.pose_delta) and torch.equal(alone.image_set.poses, both.image_set.poses)


def test_checkpoint_resumes_the_camera_sequence(gpu, tmp_path):
    torch = gpu
    kw = dict(refine_cameras=RATES, sample_jitter=True, jitter_seed=21)
    a = _trainer(torch, **kw)
    _run(a, "images", steps=3)
    path = str(tmp_path / "cameras.rtxn")
    a.save_checkpoint(path)
    _run(a, "images", steps=2)
    b = _trainer(torch, **kw)
    header = b.load_checkpoint(path)
    assert {"camera_delta", "camera_m", "camera_v", "camera_steps", "camera_skipped"} <= {e["name"] for e in header["arrays"]}
    assert float(b.camera_delta.abs().max()) > 0 and not torch.equal(b.image_set.cameras.params, b.cameras0)
    _run(b, "images", steps=2)
    _assert_same(torch, _tstate(a), _tstate(b), "resumed")
    # a file written without the refinement: the correction starts from zeros, the rows from the attached ones
    plain = _trainer(torch)
    _run(plain, "images", steps=1)
    old = str(tmp_path / "plain.rtxn")
    plain.save_checkpoint(old)
    b.load_checkpoint(old)
    assert float(b.camera_delta.abs().max()) == 0 and int(b.camera_updates.max()) == 0 and torch.equal(b.image_set.cameras.params, b.cameras0)


def test_check_cameras_judges_the_live_rows(gpu):
    torch = gpu
    tr = _trainer(torch, refine_cameras=RATES)
    _run(tr, "images", steps=2)
    tr.check_cameras()
    rows = tr.image_set.cameras.params
    rows[2, 4] = -6.0                                    # k1 = -6: the radial map folds over inside the frame
    with pytest.raises(ValueError, match=r"camera 2 \(opencv\) is not invertible over the 16 x 12 frame: at pixel"):
        tr.check_cameras()
    tr.reset_cameras()
    tr.check_cameras()


def test_the_refusals_are_messages(gpu, monkeypatch):
    torch = gpu
    from rtx_nerf_amd import train
    tr = _trainer(torch, ray_gradients=False)
    with pytest.raises(ValueError, match="refine_cameras needs a trainer built with ray_gradients=True"):
        tr.attach_images(_image_set(torch), refine_cameras=True)
    tr = _trainer(torch)
    with pytest.raises(ValueError, match="refine_cameras needs an image set built with cameras="):
        tr.attach_images(_image_set(torch, cameras=False), refine_cameras=True)
    with pytest.raises(ValueError, match="has no \\['lr'\\]"):
        tr.attach_images(_image_set(torch), refine_cameras=dict(lr=1e-3))
    with pytest.raises(ValueError, match="lr_focal"):
        tr.attach_images(_image_set(torch), refine_cameras=dict(lr_focal=-1.0))
    with pytest.raises(RuntimeError, match="reset_cameras"):
        tr.reset_cameras()
    monkeypatch.setattr(train, "_world", lambda: 2)
    with pytest.raises(ValueError, match="refine_cameras is single-GPU"):
        tr.attach_images(_image_set(torch), refine_cameras=True)
