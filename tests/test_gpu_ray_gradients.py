"""Ray gradients and pose refinement on the GPU against the float64 restatement of tests/_ray_gradient_float64.py, whose
bounds are DERIVED there, not measured, and which tests/test_ray_gradient_float64_reference.py holds to central differences.
  * the gather (rtxn_hashgrid_input_gradient_segments) over every configuration of the hash-grid sweep, REGULAR, MIDPOINT_WORLD and
    JITTER_WORLD, all segments and the live form (unlisted segments exactly 0, their NaN-filled dencT columns never read), tails of
    1 and 3 segments, two runs and the host / device unscaling bit-identical, nothing written outside the buffers;
  * the per-ray reduction, the pose gradient and the pose step (50 steps of the float64 recurrence re-seeded from the device's own
    state, images dropping in and out, the refusals, and the rays rtxn_draw_batch then generates from the updated poses);
  * the Trainer: the three stepping paths bit-identical, the defaults and lr = 0 bit-identical to the plain trainer, the feature
    beside jitter, a dynamic loss scale, a background, the regulariser and RTXN_TRAIN_LIVE_SEGMENTS=0, and a checkpoint."""
import faulthandler

import numpy as np
import pytest

import _hashgrid_float64 as H
import _ray_gradient_float64 as G

pytestmark = pytest.mark.gpu

CASES = list(H.SWEEP)
IDS = ["%dx%d-T%d-b%d-s%g" % c for c in CASES]
P = 300
SENT = -7.75
JIT = (21, 5)                     # (seed, step) of the JITTER_WORLD runs
SCALE = 128.0


@pytest.fixture(autouse=True)
def _own_timeout():
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(torch, rows):
    buf = torch.full((rows + 2, 3), SENT, device="cuda")
    return buf, buf[1:rows + 1]


def _jitter(torch, api, stype):
    if stype != 4:
        return None, None
    step = torch.full((1,), JIT[1], dtype=torch.int32, device="cuda")
    return api.sample_jitter(seed=JIT[0], step=step), step


def _positions(torch, api, seg, n, stype, jitter):
    ones, idx = _dev(torch, np.ones(n, np.int32)), _dev(torch, np.arange(n, dtype=np.int32))
    samples = torch.zeros((32 * n, 5), device="cuda")
    t = torch.zeros(32 * n, device="cuda")
    api.launchSampler(*seg, t, samples, n, 8, ones, idx, stype, jitter=jitter)
    return samples.cpu().numpy()


def _run_gather(torch, api, hg, table, seg, n, stype, denc, jitter, live_ws=None, scale_device=None):
    LF = hg.cfg.n_levels * hg.cfg.n_features
    Sp = api.padded_samples(32 * n)
    dT = np.zeros((LF, Sp), np.float16)
    dT[:, :32 * n] = denc[:32 * n, :LF].T
    gs, ds = _guarded(torch, n)
    ge, de = _guarded(torch, n)
    hg.input_gradient_segments(table, seg[0], seg[1], n, stype, _dev(torch, dT), ds, de, live_ws=live_ws, jitter=jitter,
                               loss_scale=SCALE, scale_device=scale_device)
    torch.cuda.synchronize()
    for g in (gs, ge):
        assert bool((g[0] == SENT).all()) and bool((g[-1] == SENT).all()), "wrote outside dstart / dend"
    return ds.cpu().numpy(), de.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gather_matches_float64_per_element(gpu, case):
    torch = gpu
    from rtx_nerf_amd import api
    L, F, T, base, s = case
    levels = H.geometry(L, T, base, s)
    hg = api.HashGrid(L, F, T, base, s, n_dir_freqs=0)
    table = H.case_table(levels, F, L)
    tab_d = torch.empty(table.size + 2, dtype=torch.float16, device="cuda")
    aligned = _dev(torch, table)
    tab_d[2:] = aligned                                   # [2:]: 4-byte aligned only
    sp, ep, view = H.case_segments(levels, 7, P)
    seg = tuple(_dev(torch, a) for a in (sp, ep, view))
    live = H.case_live(L, P)
    dout = torch.zeros((32 * P, 4), dtype=torch.float16, device="cuda")
    dout.view(P, 32, 4)[_dev(torch, live), 0, 0] = 1.0
    ws = api.live_segments_workspace(P)
    api.live_segments(dout, P, P, ws)
    name = IDS[CASES.index(case)]
    for stype in (0, 3, 4):
        jitter, _keep = _jitter(torch, api, stype)
        x = _positions(torch, api, seg, P, stype, jitter)
        u = G.sample_u(stype, P, JIT)
        want_x = sp.astype(np.float64).repeat(32, 0) + u[:, None] * (ep.astype(np.float64) - sp.astype(np.float64)).repeat(32, 0)
        assert np.abs(x[:, :3] - want_x).max() <= 2.0 ** -22       # the restated u is the sampler's
        for form in ("all", "live"):
            d, zeroed = H.case_gradient(levels, F, x, L + stype, live if form == "live" else None)
            assert zeroed <= 0.02, (name, stype, zeroed)
            rs, re, bs, be = G.gather(levels, F, table, x, u, d, k=1.0 / SCALE)
            assert np.count_nonzero(rs) > 0
            sent = d.copy()
            if form == "live":                            # what the MLP backward leaves there is not defined: make it poison
                sent.reshape(P, 32, -1)[~live] = np.nan
            got = _run_gather(torch, api, hg, aligned, seg, P, stype, sent, jitter, ws if form == "live" else None)
            for which, g, r, b in (("dstart", got[0], rs, bs), ("dend", got[1], re, be)):
                ratio, bad = G.check(g, r, b)
                print(f"measured gather {name} stype {stype} {form} {which}: err / bound {ratio:.3f}, near-face pairs zeroed {zeroed:.4f}")
                assert bad == 0 and ratio <= 1.0, (name, stype, form, which, ratio, bad)
            if form == "live":
                assert np.all(got[0][~live] == 0.0) and np.all(got[1][~live] == 0.0)
            again = _run_gather(torch, api, hg, aligned, seg, P, stype, sent, jitter, ws if form == "live" else None)
            assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
            if form == "all":
                word = torch.full((1,), SCALE, device="cuda")
                dev = _run_gather(torch, api, hg, aligned, seg, P, stype, sent, jitter, scale_device=word)
                assert got[0].tobytes() == dev[0].tobytes() and got[1].tobytes() == dev[1].tobytes()
                if F > 1:                                 # a table that is 4-byte aligned only: the same bits
                    other = _run_gather(torch, api, hg, tab_d[2:], seg, P, stype, sent, jitter)
                    assert got[0].tobytes() == other[0].tobytes() and got[1].tobytes() == other[1].tobytes()
                if stype == 3:
                    for n in (1, 3):                      # half a wave, and one and a half
                        tail = _run_gather(torch, api, hg, aligned, seg, n, stype, sent, jitter)
                        for g, r, b in ((tail[0], rs[:n], bs[:n]), (tail[1], re[:n], be[:n])):
                            ratio, bad = G.check(g, r, b)
                            assert bad == 0 and ratio <= 1.0, (name, "tail", n, ratio, bad)


# ------------------------------------------------------------------------------------------------ the per-ray reduction
@pytest.mark.parametrize("n_rays", [1, 63, 65])
def test_ray_reduction_matches_float64(gpu, n_rays):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(n_rays)
    pattern_hits = [70, 0, 1, 2, 33, 9]
    pattern_stored = [70, 0, 1, 2, 33, 5]                 # the last one truncated: num_stored < num_hits
    hits = np.array([pattern_hits[r % 6] for r in range(n_rays)], np.int32)
    stored = np.array([pattern_stored[r % 6] for r in range(n_rays)], np.int32)
    indices = np.concatenate([[0], np.cumsum(hits)[:-1]]).astype(np.int32)
    M = int(hits.sum())
    t = np.sort(rng.uniform(0.05, 3.0, (M, 2)), axis=1).astype(np.float32)
    ds, de = (rng.standard_normal((M, 3)) * 1e-3).astype(np.float32), (rng.standard_normal((M, 3)) * 1e-3).astype(np.float32)
    for r in range(n_rays):                               # slots a truncated ray never stored: poison
        ds[indices[r] + stored[r]:indices[r] + hits[r]] = np.nan
    go, o = _guarded(torch, n_rays)
    gd, d = _guarded(torch, n_rays)
    args = [_dev(torch, a) for a in (indices, stored, t[:, 0], t[:, 1], ds, de)]
    api.ray_gradients_reduce(*args, n_rays, o, d)
    torch.cuda.synchronize()
    for g in (go, gd):
        assert bool((g[0] == SENT).all()) and bool((g[-1] == SENT).all())
    want_o, want_d, bo, bd = G.ray_reduce(indices, stored, t[:, 0], t[:, 1], ds, de)
    for which, got, want, b in (("d_origin", o, want_o, bo), ("d_direction", d, want_d, bd)):
        ratio, bad = G.check(got.cpu().numpy(), want, b)
        print(f"measured ray reduction {n_rays} rays {which}: err / bound {ratio:.3f}")
        assert bad == 0 and ratio <= 1.0, (which, ratio, bad)
    assert np.all(o.cpu().numpy()[stored == 0] == 0.0) and np.all(d.cpu().numpy()[stored == 0] == 0.0)
    o2, d2 = torch.zeros_like(o), torch.zeros_like(d)
    api.ray_gradients_reduce(*args, n_rays, o2, d2)
    assert torch.equal(o, o2) and torch.equal(d, d2)


# ------------------------------------------------------------------------------------------------ the pose gradient and step
def _pose_state(torch, api, n, poses0, skip=None, **cfg):
    st = dict(poses0=_dev(torch, poses0), poses=_dev(torch, poses0).clone(), delta=torch.zeros((n, 6), device="cuda"),
              m=torch.zeros((n, 6), device="cuda"), v=torch.zeros((n, 6), device="cuda"),
              steps=torch.zeros(n, dtype=torch.int32, device="cuda"), grad=torch.zeros((n, 8), device="cuda"),
              skipped=torch.zeros(1, dtype=torch.int32, device="cuda"))
    return st, api.pose_refinement(n, **cfg, skip=skip, **st)


def _poses0(n):
    from rtx_nerf_amd import scenes
    return np.stack([np.asarray(scenes.pose_spherical(35.0 + 80.0 * i, -25.0 - 10.0 * i, origin_scale=10.0), np.float32).reshape(16)
                     for i in range(n)])


@pytest.mark.parametrize("n_rays", [1, 255, 257])
def test_pose_gradient_matches_float64(gpu, n_rays):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(n_rays)
    st, pose = _pose_state(torch, api, 3, _poses0(3))
    st["grad"].fill_(SENT)
    drawn = np.stack([rng.integers(0, 2, n_rays), rng.integers(0, 192, n_rays)], 1).astype(np.int32)      # image 2 is never drawn
    d = rng.standard_normal((n_rays, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    go, gd = (rng.standard_normal((n_rays, 3)) * 1e-5).astype(np.float32), (rng.standard_normal((n_rays, 3)) * 1e-5).astype(np.float32)
    args = [_dev(torch, a) for a in (drawn, d, go, gd)]
    api.pose_gradients(*args, n_rays, pose)
    got = st["grad"].cpu().numpy()
    want, bound = G.pose_gradients(drawn[:, 0], d, go, gd, 3)
    ratio, bad = G.check(got[:, :6], want[:, :6], bound[:, :6])
    print(f"measured pose gradient {n_rays} rays: err / bound {ratio:.3f}")
    assert bad == 0 and ratio <= 1.0
    assert np.array_equal(got[:, 6], want[:, 6]) and np.all(got[:, 7] == 0.0) and np.all(got[2] == 0.0)
    st["grad"].fill_(SENT)
    api.pose_gradients(*args, n_rays, pose)
    assert st["grad"].cpu().numpy().tobytes() == got.tobytes()


def test_pose_step_follows_the_float64_recurrence(gpu):
    torch = gpu
    from rtx_nerf_amd import api
    N, cfg = 4, dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15)
    poses0 = _poses0(N)
    poses0[1, 12] = -0.0                                  # a signed zero survives the copy
    st, pose = _pose_state(torch, api, N, poses0, **cfg)
    api.pose_compose(pose)
    assert st["poses"].cpu().numpy().tobytes() == poses0.tobytes()          # delta == 0: poses0 bit for bit
    rng = np.random.default_rng(50)
    names = ("delta", "m", "v", "steps", "poses")
    worst = dict(delta=0.0, m=0.0, v=0.0, pose=0.0)
    for step in range(50):
        grad = np.zeros((N, 8), np.float32)
        grad[:, :6] = rng.standard_normal((N, 6)) * 10.0 ** rng.uniform(-8, -5, (N, 1))
        grad[:, 6] = rng.integers(0, 3, N) * (rng.random(N) < 0.7)           # images drop in and out of the batch
        grad[0, 6] = 5 if step % 2 == 0 else 0
        st["grad"].copy_(_dev(torch, grad))
        before = {k: st[k].cpu().numpy() for k in names}
        api.pose_step(pose)
        after = {k: st[k].cpu().numpy() for k in names}
        for i in range(N):
            if grad[i, 6] == 0:
                assert all(before[k][i].tobytes() == after[k][i].tobytes() for k in names), (step, i)
                continue
            d1, m1, v1, t, b_d, b_m, b_v = G.adam_update(before["delta"][i], before["m"][i], before["v"][i], before["steps"][i], grad[i, :6], **cfg)
            assert after["steps"][i] == t
            for k, got, want, b in (("delta", after["delta"][i], d1, b_d), ("m", after["m"][i], m1, b_m), ("v", after["v"][i], v1, b_v)):
                ratio, bad = G.check(got, want, b)
                worst[k] = max(worst[k], ratio)
                assert bad == 0, (step, i, k, ratio)
            want, b = G.compose_pose(poses0[i], after["delta"][i])
            ratio, bad = G.check(after["poses"][i].reshape(4, 4), want, b)
            worst["pose"] = max(worst["pose"], ratio)
            assert bad == 0, (step, i, "pose", ratio)
    print("measured pose step, worst err / bound over 50 steps: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert int(st["steps"].max()) > 10 and float(st["delta"].abs().max()) > 1e-3 and int(st["skipped"].item()) == 0
    # a non-finite gradient: that image keeps every word and the count goes up; the others step
    grad = np.zeros((N, 8), np.float32)
    grad[:, :6], grad[:, 6] = 1e-6, 2
    grad[1, 2] = np.nan
    st["grad"].copy_(_dev(torch, grad))
    before = {k: st[k].cpu().numpy() for k in names}
    api.pose_step(pose)
    after = {k: st[k].cpu().numpy() for k in names}
    assert all(before[k][1].tobytes() == after[k][1].tobytes() for k in names) and int(st["skipped"].item()) == 1
    assert after["steps"][0] == before["steps"][0] + 1 and after["delta"][0].tobytes() != before["delta"][0].tobytes()
    # the guard's skip word: nothing moves for any image, and nothing is counted
    skip = torch.ones(1, dtype=torch.int32, device="cuda")
    guarded = api.pose_refinement(N, **cfg, skip=skip, **st)
    before = {k: st[k].cpu().numpy() for k in names}
    api.pose_step(guarded)
    after = {k: st[k].cpu().numpy() for k in names}
    assert all(before[k].tobytes() == after[k].tobytes() for k in names) and int(st["skipped"].item()) == 1
    # the next draw generates its rays from the updated poses
    W, Hh, focal = 16, 12, 1.3
    images = torch.zeros((N, Hh, W, 3), device="cuda")
    iset = api.ImageSet(images, st["poses"], focal)
    n = 512
    o, d, tg = torch.zeros((n, 3), device="cuda"), torch.zeros((n, 3), device="cuda"), torch.zeros((n, 3), device="cuda")
    dr = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    api.draw_batch(iset, n, 3, None, o, d, tg, dr)
    o, d, dr = o.cpu().numpy().astype(np.float64), d.cpu().numpy().astype(np.float64), dr.cpu().numpy()
    delta = st["delta"].cpu().numpy()
    assert np.abs(delta[:, :3]).max() > 1e-3
    for r in range(n):
        i, pix = int(dr[r, 0]), int(dr[r, 1])
        pose64, b = G.compose_pose(poses0[i], delta[i])
        wo, wd = G.make_ray(pose64, focal, W / Hh, W, Hh, pix % W, pix // W)
        assert np.all(np.abs(o[r] - wo) <= b[:3, 3] / 10 + G.U * np.abs(wo)), (r, o[r], wo)      # the composition's own rounding, and the / 10
        assert np.abs(d[r] - wd).max() <= 2e-6, (r, np.abs(d[r] - wd).max())


# ------------------------------------------------------------------------------------------------ the Trainer
R, B, N_IMG, W, HGT = 16, 256, 4, 16, 12
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)


def _image_set(torch, channels=3):
    """a fresh set every time: the refinement rewrites its poses in place"""
    from rtx_nerf_amd import api, scenes
    img = np.random.default_rng(100 + channels).uniform(0, 1, (N_IMG, HGT, W, channels)).astype(np.float32)
    return api.ImageSet(torch.from_numpy(img).cuda(), torch.from_numpy(_poses0(N_IMG)).cuda(), scenes.lego_focal_length(True))


def _trainer(torch, refine=None, channels=3, **kw):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()
    args = dict(lr=1e-2, loss_scale=128.0, density_scale=120.0, mode="nerf", seed=3, deterministic=True)
    args.update(kw)
    tr = Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=2, hashgrid=HGD, n_dir_freqs=4, batch_rays=B, max_segments=B * 30, **args)
    tr.attach_images(_image_set(torch, channels), refine_poses=refine)
    return tr


def _run(tr, path, steps=5):
    if path == "captured":
        tr.capture_step(B, launch_segments=B * 30, draw=True)
    elif path == "entry":
        tr.entry_args(B, launch_segments=B * 30, draw=True)
    fn = {"images": tr.step_images, "captured": tr.step_captured, "entry": tr.step_entry}[path]
    return [float(fn().item()) for _ in range(steps)]


def _state(tr):
    out = dict(params=tr.params, master=tr.master, table=tr.table, table_master=tr.table_master, poses=tr.image_set.poses)
    if tr._pose is not None:
        out.update(pose_delta=tr.pose_delta, pose_updates=tr.pose_updates, pose_m=tr._pose_m, pose_v=tr._pose_v)
    if tr.ray_gradients:
        out.update(rays_o_grad=tr.rays_o_grad, rays_d_grad=tr.rays_d_grad)
    return {k: v.clone() for k, v in out.items()}


def _assert_same(torch, a, b, what, keys=None):
    for k in (keys or a.keys()):
        assert torch.equal(a[k], b[k]), f"{what}: {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} differ"


def test_trainer_ray_gradients_equal_the_direct_calls(gpu):
    torch = gpu
    from rtx_nerf_amd import api
    tr = _trainer(torch, ray_gradients=True, sample_jitter=True, jitter_seed=21)
    o, d, t = (torch.zeros((B, c), device="cuda") for c in (3, 3, 3))
    api.draw_batch(tr.image_set, B, 0, None, o, d, t)
    table0 = tr.table.clone()
    tr.step(o, d, t)
    got_o, got_d = tr.rays_o_grad.clone(), tr.rays_d_grad.clone()
    Pn = int(tr.total.item())
    assert Pn > B
    ds, de = torch.full_like(tr.dstart, SENT), torch.full_like(tr.dend, SENT)
    ro, rd = torch.zeros_like(got_o), torch.zeros_like(got_d)
    jit = tr._jitter(tr._jit_step)
    api.hashgrid_input_gradient_segments(tr.hg, table0, tr.start, tr.end, Pn, api.SAMPLING_JITTER_WORLD, tr.dencT, ds, de, live_ws=tr.live_ws,
                                         jitter=jit, loss_scale=tr.loss_scale)
    api.ray_gradients_reduce(tr.indices, tr.num_stored, tr.t_start, tr.t_end, ds, de, B, ro, rd)
    assert torch.equal(ds[:Pn], tr.dstart[:Pn]) and torch.equal(ro, got_o) and torch.equal(rd, got_d)
    assert bool(torch.isfinite(got_o).all()) and bool(torch.isfinite(got_d).all())
    assert int((got_o.abs().sum(1) > 0).sum()) > B // 8 and float(got_d.abs().max()) > 0
    hit = tr.num_stored[:B] > 0
    assert bool((got_o[~hit] == 0).all()) and bool((got_d[~hit] == 0).all())
    stages = tr.time_stages(o, d, t, steps=1)
    assert "ray_grad" in stages and "hash_bwd" in stages


def test_three_stepping_paths_refine_the_same_poses(gpu):
    torch = gpu
    got = {}
    for path in ("images", "captured", "entry"):
        tr = _trainer(torch, refine=dict(lr=1e-3), ray_gradients=True, sample_jitter=True, jitter_seed=21)
        if path == "captured":
            poses_before = tr.image_set.poses.clone()
            tr.capture_step(B, launch_segments=B * 30, draw=True)
            assert torch.equal(tr.image_set.poses, poses_before) and int(tr.pose_updates.max()) == 0      # the warm-up is no step
            losses = [float(tr.step_captured().item()) for _ in range(5)]
        else:
            losses = _run(tr, path)
        got[path] = (_state(tr), losses)
        assert int(tr.pose_updates.min()) >= 4 and float(tr.pose_delta.abs().max()) > 1e-3 and int(tr.pose_skipped.item()) == 0
        assert not torch.equal(tr.refined_poses().view(-1, 16), tr.poses0)
        assert torch.equal(tr.refined_poses().view(-1, 16)[:, 12:], tr.poses0[:, 12:])
    for path in ("captured", "entry"):
        _assert_same(torch, got["images"][0], got[path][0], path)
        assert got["images"][1] == got[path][1], path
    tr.reset_poses()
    assert torch.equal(tr.image_set.poses, tr.poses0) and int(tr.pose_updates.max()) == 0 and float(tr.pose_delta.abs().max()) == 0


def test_defaults_and_zero_rate_leave_the_run_bit_identical(gpu):
    torch = gpu
    keys = ("params", "master", "table", "table_master", "poses")
    plain = _trainer(torch)
    assert plain._rays is None and plain.rays_o_grad is None and plain.t_start is None and plain._pose is None
    want_losses = _run(plain, "images")
    want = _state(plain)
    for path in ("images", "captured", "entry"):
        for refine in (None, dict(lr=0.0)):
            tr = _trainer(torch, refine=refine, ray_gradients=True)
            losses = _run(tr, path)
            _assert_same(torch, want, _state(tr), f"{path}, refine_poses={refine}", keys)
            assert losses == want_losses, (path, refine)
            if refine is not None:
                assert float(tr.pose_delta.abs().max()) == 0 and int(tr.pose_updates.min()) >= 4


@pytest.mark.parametrize("config", ["everything", "every_segment"])
def test_refinement_beside_the_other_training_options(gpu, config, monkeypatch):
    torch = gpu
    if config == "everything":
        kw = dict(sample_jitter=True, jitter_seed=5, loss_scale="dynamic", background=(1.0, 1.0, 1.0), target_channels=4, distortion_weight=0.01, ema_decay=0.9)
        channels = 4
    else:
        monkeypatch.setenv("RTXN_TRAIN_LIVE_SEGMENTS", "0")
        kw, channels = {}, 3
    got = {}
    for path in ("images", "captured", "entry"):
        tr = _trainer(torch, refine=True, channels=channels, ray_gradients=True, **kw)
        assert tr.live_segments == (config == "everything")
        if config == "everything":
            assert tr._reg.t_start == tr._rays.t_start and tr._reg.t_end == tr._rays.t_end          # one pair of buffers
        losses = _run(tr, path, steps=3)
        got[path] = (_state(tr), losses)
        assert all(np.isfinite(losses)) and float(tr.pose_delta.abs().max()) > 0 and bool(torch.isfinite(tr.image_set.poses).all())
    for path in ("captured", "entry"):
        _assert_same(torch, got["images"][0], got[path][0], f"{config}: {path}")
        assert got["images"][1] == got[path][1], (config, path)


def test_checkpoint_resumes_the_pose_sequence(gpu, tmp_path):
    torch = gpu
    kw = dict(refine=dict(lr=2e-3), ray_gradients=True, sample_jitter=True, jitter_seed=21)
    a = _trainer(torch, **kw)
    _run(a, "images", steps=3)
    path = str(tmp_path / "pose.rtxn")
    a.save_checkpoint(path)
    _run(a, "images", steps=2)
    b = _trainer(torch, **kw)
    header = b.load_checkpoint(path)
    assert {"pose_delta", "pose_m", "pose_v", "pose_steps", "pose_skipped"} <= {e["name"] for e in header["arrays"]}
    assert float(b.pose_delta.abs().max()) > 0 and not torch.equal(b.image_set.poses, b.poses0)
    _run(b, "images", steps=2)
    _assert_same(torch, _state(a), _state(b), "resumed")
    # a file written without the refinement: the correction starts from zeros, the poses from the attached ones
    plain = _trainer(torch)
    _run(plain, "images", steps=1)
    old = str(tmp_path / "plain.rtxn")
    plain.save_checkpoint(old)
    b.load_checkpoint(old)
    assert float(b.pose_delta.abs().max()) == 0 and int(b.pose_updates.max()) == 0 and torch.equal(b.image_set.poses, b.poses0)
