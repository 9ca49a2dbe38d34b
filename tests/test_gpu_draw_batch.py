"""Training batches drawn on the device (rtxn_draw_batch): the hash against a numpy restatement of include/rtxn.h, the
targets against the stored frames, the rays against the pinhole traversal they must reproduce and against camera_rays, the
coverage of the draw, and the Trainer's three stepping paths fed from the image set against a trainer fed the same batches by hand.

Shapes: 3 frames of 16 x 12 (not square, so x and y cannot be swapped unnoticed; 576 pixels), distinct poses, random content;
batches of 1, 257 (a tail block of one ray), 4096 and 65536 rays; the trainer tests use the tiny hash model of
test_gpu_sample_jitter.py on 256 rays."""
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_IMG, W, H = 3, 16, 12
NPIX = W * H
U32, U64 = np.uint32, np.uint64
PAIRS = [(0, 0), (0, 1), (7, 5)]            # (seed, step)
R, B = 16, 256
HGD = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)


@pytest.fixture(autouse=True)
def _own_timeout():
    """every test here under its own limit: a hung kernel ends the run (with every thread's stack) instead of stalling it"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- the definition, restated (include/rtxn.h, "training batches drawn on the device") ------------------------------------
def fmix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> U32(16)
    h *= U32(0x85EBCA6B)
    h ^= h >> U32(13)
    h *= U32(0xC2B2AE35)
    h ^= h >> U32(16)
    return h


def drawn_cpu(seed, step, n, n_images=N_IMG, n_pixels=NPIX):
    """[n, 2] (image, pixel) of batch `step` in uint64 arithmetic"""
    with np.errstate(over="ignore"):
        h0 = fmix32((U32(seed) ^ U32(0x2C1B3C6D)) + U32(0x9E3779B9) * U32(step))
        r = np.arange(n, dtype=np.uint32)
        hi, hp = fmix32(h0 ^ (U32(2) * r)), fmix32(h0 ^ (U32(2) * r + U32(1)))
    image = (hi.astype(U64) * U64(n_images)) >> U64(32)
    pixel = (hp.astype(U64) * U64(n_pixels)) >> U64(32)
    return np.stack([image, pixel], axis=1).astype(np.int64)


_CACHE = {}


def _poses():
    from rtx_nerf_amd import scenes
    return np.stack([np.asarray(scenes.pose_spherical(35.0 + 110.0 * i, -25.0 - 10.0 * i, origin_scale=10.0), np.float32).reshape(16)
                     for i in range(N_IMG)])


def _frames(channels, u8):
    rng = np.random.default_rng(100 + channels + 10 * u8)
    if u8:
        return rng.integers(0, 256, (N_IMG, H, W, channels), dtype=np.uint8)
    return rng.uniform(0, 1, (N_IMG, H, W, channels)).astype(np.float32)


def _set(torch, channels=3, u8=False):
    """(api.ImageSet, frames as numpy), made once per layout"""
    key = ("set", channels, u8)
    if key not in _CACHE:
        from rtx_nerf_amd import api, scenes
        img = _frames(channels, u8)
        _CACHE[key] = (api.ImageSet(torch.from_numpy(img).cuda(), torch.from_numpy(_poses()).cuda(), scenes.lego_focal_length(True)), img)
    return _CACHE[key]


def _draw(torch, iset, n, seed, step, with_drawn=True):
    """one api.draw_batch into fresh buffers pre-filled with a guard value; -> rays_o, rays_d, targets, drawn (device tensors)"""
    from rtx_nerf_amd import api
    o = torch.full((n + 3, 3), -7.0, device="cuda")
    d = torch.full((n + 3, 3), -7.0, device="cuda")
    t = torch.full((n + 3, iset.channels), -7.0, device="cuda")
    dr = torch.full((n + 3, 2), -7, dtype=torch.int32, device="cuda") if with_drawn else None
    st = None if step is None else torch.full((1,), step, dtype=torch.int32, device="cuda")
    api.draw_batch(iset, n, seed, st, o, d, t, dr)
    torch.cuda.synchronize()
    for buf in (o, d, t) + ((dr,) if with_drawn else ()):                   # nothing past ray n - 1 is written (the tail block)
        assert bool((buf[n:] == -7).all())
    return o[:n], d[:n], t[:n], (dr[:n] if with_drawn else None)


# ---- 1. the hash -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 4096])
def test_drawn_equals_the_restated_hash(gpu, n):
    torch = gpu
    iset, _ = _set(torch)
    for seed, step in PAIRS:
        _, _, _, dr = _draw(torch, iset, n, seed, step)
        np.testing.assert_array_equal(dr.cpu().numpy().astype(np.int64), drawn_cpu(seed, step, n), err_msg=f"seed {seed} step {step}")
    # a NULL step is step 0
    np.testing.assert_array_equal(_draw(torch, iset, n, 7, None)[3].cpu().numpy(), drawn_cpu(7, 0, n))


def test_consecutive_batches_share_almost_nothing(gpu):
    torch = gpu
    iset, _ = _set(torch)
    a = _draw(torch, iset, 4096, 0, 0)[3].cpu().numpy()
    b = _draw(torch, iset, 4096, 0, 1)[3].cpu().numpy()
    share = float((a == b).all(axis=1).mean())
    print(f"rays equal in batches 0 and 1: {100 * share:.3f} % (restated on the CPU: 0.049 %; chance: 1/1728 = 0.058 %)")
    assert share < 0.01


# ---- 2. targets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_targets_are_the_stored_pixels_bit_for_bit(gpu, channels, u8):
    torch = gpu
    iset, img = _set(torch, channels, u8)
    for n, (seed, step) in ((4096, PAIRS[2]), (257, PAIRS[1])):
        _, _, t, dr = _draw(torch, iset, n, seed, step)
        dr = dr.cpu().numpy()
        np.testing.assert_array_equal(dr, drawn_cpu(seed, step, n))
        px = img[dr[:, 0], dr[:, 1] // W, dr[:, 1] % W]                       # [n, C]
        want = px.astype(np.float32) / np.float32(255.0) if u8 else px        # numpy float32 division: IEEE, as the kernel's
        assert want.dtype == np.float32 and want.shape == (n, channels)
        np.testing.assert_array_equal(t.cpu().numpy(), want)
        # the draw without the optional `drawn` output writes the same rays and targets
        o2, d2, t2, _ = _draw(torch, iset, n, seed, step, with_drawn=False)
        assert torch.equal(t2, t)


# ---- 3. rays -----------------------------------------------------------------------------------------------------------------
def _trace_packed(torch, n, **rays):
    """count -> scan -> write (dense grid 16, DDA, packed); everything the traversal says about the rays, as numpy"""
    from rtx_nerf_amd import api
    kw = dict(grid_res=R, mode=api.TRACE_DDA, **rays)
    nh = torch.zeros(n, dtype=torch.int32, device="cuda")
    org = torch.zeros((n, 3), device="cuda")
    vd = torch.zeros((n, 2), device="cuda")
    api.trace_grid(num_hits=nh, **kw)
    idx, total = api.scan_hits(nh)
    P = int(total.item())
    sp, ep = torch.zeros((P, 3), device="cuda"), torch.zeros((P, 3), device="cuda")
    api.trace_grid(num_hits=nh, ray_origins=org, viewing_direction=vd, indices=idx, start_points=sp, end_points=ep, segment_capacity=P, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(num_hits=nh, origins=org, view=vd, indices=idx, start=sp, end=ep).items()}


def test_drawn_rays_walk_the_grid_as_the_pinhole_launch_does(gpu):
    """rtxn_trace_grid over each frame's whole 16 x 12 pinhole launch, and over the 4096 drawn rays as explicit rays: origin,
    viewing direction, segment count and every segment's end points of a drawn ray are those of its pixel's pinhole ray, bit for
    bit -- the draw generates rays with the traversal's own function."""
    torch = gpu
    from rtx_nerf_amd import scenes
    iset, _ = _set(torch)
    f, n = scenes.lego_focal_length(True), 4096
    pin = [_trace_packed(torch, NPIX, look_at=iset.poses[i], focal_length=f, aspect_ratio=W / H, width=W, height=H) for i in range(N_IMG)]
    assert all(p["num_hits"].max() > 0 for p in pin)
    o, d, _, dr = _draw(torch, iset, n, 7, 5)
    exp = _trace_packed(torch, n, rays_o=o.contiguous(), rays_d=d.contiguous())
    dr = dr.cpu().numpy()
    assert exp["num_hits"].sum() > n                               # the batch does cross the grid
    segs = 0
    for i in range(N_IMG):
        rays = np.nonzero(dr[:, 0] == i)[0]
        pix = dr[rays, 1]
        assert rays.size > 1000
        np.testing.assert_array_equal(exp["origins"][rays], pin[i]["origins"][pix])
        np.testing.assert_array_equal(exp["view"][rays], pin[i]["view"][pix])
        np.testing.assert_array_equal(exp["num_hits"][rays], pin[i]["num_hits"][pix])
        cnt = exp["num_hits"][rays].astype(np.int64)
        within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)          # 0 .. cnt-1 per ray
        mine = np.repeat(exp["indices"][rays].astype(np.int64), cnt) + within
        theirs = np.repeat(pin[i]["indices"][pix].astype(np.int64), cnt) + within
        for k in ("start", "end"):
            np.testing.assert_array_equal(exp[k][mine], pin[i][k][theirs], err_msg=f"frame {i}: {k}_points")
        segs += int(cnt.sum())
    assert segs == int(exp["num_hits"].sum())
    # rays_o is the origin the traversal reports, as stored
    np.testing.assert_array_equal(o.cpu().numpy(), exp["origins"])


def test_ray_directions_against_camera_rays(gpu):
    """rays_d (and rays_o) against camera_rays, which forms the same pinhole rays in float64.  Tolerance: the absolute 2e-6 that
    test_gpu_parity.py allows the pinhole launch's viewing directions against the oracle (_assert_trace_equal) -- an angle of a
    unit vector and its components move alike.  Unit length to the same bound."""
    torch = gpu
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    iset, _ = _set(torch)
    o, d, _, dr = _draw(torch, iset, 4096, 0, 1)
    o, d, dr = o.cpu().numpy(), d.cpu().numpy(), dr.cpu().numpy()
    poses = _poses()
    want_o, want_d = np.zeros_like(o), np.zeros_like(d)
    for i in range(N_IMG):
        co, cd = camera_rays(poses[i], scenes.lego_focal_length(True), W, H, device="cpu")
        m = dr[:, 0] == i
        want_o[m], want_d[m] = co.numpy()[dr[m, 1]], cd.numpy()[dr[m, 1]]
    err_d, err_o = np.abs(d - want_d).max(), np.abs(o - want_o).max()
    print(f"max |rays_d - camera_rays| = {err_d:.3e}, max |rays_o - camera_rays| = {err_o:.3e} (bound 2e-6)")
    assert err_d <= 2e-6 and err_o <= 2e-6
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 2e-6


# ---- 4. coverage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", PAIRS + [(123, 1000)])
def test_every_pixel_is_drawn_about_equally_often(gpu, seed, step):
    """n = 65536 over 3 x 192 pixels: mean 113.8 per pixel, every one within +-50 % (57 .. 171; the CPU restatement gives 76 .. 150
    over these four pairs), and every frame within +-3 % of n / 3."""
    torch = gpu
    iset, _ = _set(torch)
    n = 65536
    dr = _draw(torch, iset, n, seed, step)[3].cpu().numpy().astype(np.int64)
    assert dr[:, 0].min() >= 0 and dr[:, 0].max() < N_IMG and dr[:, 1].min() >= 0 and dr[:, 1].max() < NPIX
    per_pixel = np.bincount(dr[:, 0] * NPIX + dr[:, 1], minlength=N_IMG * NPIX)
    per_image = np.bincount(dr[:, 0], minlength=N_IMG)
    print(f"seed {seed} step {step}: per pixel {per_pixel.min()} .. {per_pixel.max()}, per frame {per_image.tolist()}")
    assert per_pixel.size == N_IMG * NPIX and per_pixel.min() >= 57 and per_pixel.max() <= 171
    assert np.abs(per_image - n / 3).max() <= 0.03 * n / 3


# ---- 5. the trainer ------------------------------------------------------------------------------------------------------------
def _trainer(torch, attach=True, **kw):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()
    tr = Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=4, hashgrid=HGD, n_dir_freqs=4, batch_rays=B, max_segments=B * 30,
                 lr=1e-2, loss_scale=128.0, density_scale=120.0, mode="nerf", seed=3, deterministic=True, sample_jitter=True, jitter_seed=21, **kw)
    if attach:
        tr.attach_images(_set(torch)[0])
    return tr


def _state(tr):
    return [t.clone() for t in (tr.params, tr.master, tr.table, tr.table_master)]


def _reference(torch):
    """trainer B: no image set; step() on the batches api.draw_batch returns for counters 0, 1, 2 (seed 0).  Made once, never
    changed: the batches, the losses and the state after every step."""
    if "ref" not in _CACHE:
        iset, _ = _set(torch)
        b = _trainer(torch, attach=False)
        batches, losses, states = [], [], []
        for k in range(3):
            o, d, t, dr = _draw(torch, iset, B, 0, k)
            batches.append((o.clone(), d.clone(), t.clone(), dr.clone()))
            losses.append(float(b.step(o, d, t).item()))
            assert int(b.total.item()) > B                      # the batch crosses the occupied sphere
            states.append(_state(b))
        assert b.step_count == 3 and losses[0] > 0 and not torch.equal(states[0][1], states[2][1])
        _CACHE["ref"] = (batches, losses, states)
    return _CACHE["ref"]


def _same(torch, tr, want, what):
    for name, x, y in zip(("params", "master", "table", "table_master"), _state(tr), want):
        assert torch.equal(x, y), f"{what}: {name}: {int((x != y).sum())} of {x.numel()} differ"


def test_step_images_equals_step_on_the_same_batches(gpu):
    torch = gpu
    batches, losses, states = _reference(torch)
    a = _trainer(torch)
    for k in range(3):
        loss = float(a.step_images().item())
        assert torch.equal(a.drawn[:B], batches[k][3]) and torch.equal(a.draw_rays_o[:B], batches[k][0])
        assert torch.equal(a.draw_rays_d[:B], batches[k][1]) and torch.equal(a.draw_targets[:B], batches[k][2])
        assert abs(loss - losses[k]) <= 1e-6 * losses[k]          # a sanity bar only; bit equality: test_losses_equal_trainer_b_bit_for_bit
        _same(torch, a, states[k], f"step_images, step {k}")
    assert a.draw_count == 3 and int(a._draw_step.item()) == 3 and a.step_count == 3


@pytest.mark.parametrize("prefetch", [False, True], ids=["serial", "prefetch"])
def test_captured_step_draws_the_same_batches(gpu, prefetch):
    """capture_step(draw=True): nothing is filled in; parameters and losses equal trainer B's bit for bit after every step (the
    standard test_gpu_sample_jitter.py holds step_captured() to).  With prefetch the loss of batch k arrives a call later and
    flush_captured() trains on the last batch."""
    torch = gpu
    batches, losses, states = _reference(torch)
    a = _trainer(torch)
    a.capture_step(B, launch_segments=B * 30, prefetch=prefetch, draw=True)
    assert a.draw_count == 0 and int(a._draw_step.item()) == 0 and a.step_count == 0       # the capture's warm-up drew nothing
    got = []
    if prefetch:
        assert a.step_captured() is None                        # draws and traverses batch 0
    for k in range(3):
        loss = a.step_captured() if (not prefetch or k < 2) else a.flush_captured()
        got.append(float(loss.item()))
        _same(torch, a, states[k], f"step_captured(prefetch={prefetch}), step {k}")
    assert a.draw_count == 3 and int(a._draw_step.item()) == 3 and a.step_count == 3
    assert torch.equal(a.drawn[:B], batches[2][3])


def test_one_call_step_draws_the_same_batches(gpu):
    """entry_args(draw=True) + step_entry(): rtxn_draw_batch in front of rtxn_train_step_jitter; bit for bit trainer B."""
    torch = gpu
    from rtx_nerf_amd import _lib
    batches, losses, states = _reference(torch)
    a = _trainer(torch)
    args, dargs = a.entry_args(B, launch_segments=B * 30, draw=True)
    assert isinstance(args, _lib.TrainStepArgs) and isinstance(dargs, _lib.DrawBatchArgs)
    assert dargs.n_rays == B and dargs.rays_o == a.graph_rays_o.data_ptr() and dargs.targets == a.graph_targets.data_ptr()
    for k in range(3):
        loss = float(a.step_entry().item())
        assert torch.equal(a.graph_rays_d, batches[k][1]) and torch.equal(a.graph_targets, batches[k][2])
        _same(torch, a, states[k], f"step_entry, step {k}")
    assert a.draw_count == 3 and int(a._draw_step.item()) == 3


def _losses_of(torch, path):
    a = _trainer(torch)
    if path == "step_images":
        return [float(a.step_images().item()) for _ in range(3)]
    if path == "step_entry":
        a.entry_args(B, launch_segments=B * 30, draw=True)
        return [float(a.step_entry().item()) for _ in range(3)]
    prefetch = path == "captured_prefetch"
    a.capture_step(B, launch_segments=B * 30, prefetch=prefetch, draw=True)
    if prefetch:
        a.step_captured()
    return [float((a.step_captured() if (not prefetch or k < 2) else a.flush_captured()).item()) for k in range(3)]


@pytest.mark.parametrize("path", ["step_images", "captured", "captured_prefetch", "step_entry"])
def test_losses_equal_trainer_b_bit_for_bit(gpu, path):
    """The loss scalars of the three steps, bit for bit trainer B's.  The trainers run in deterministic mode, in which the training
    compositor's loss is summed in a fixed order behind the kernel (loss.hip) instead of by the compositor's float atomics -- with the
    atomics the scalar's last bit followed the order the blocks retired in (measured: one float32 ulp, 2.98e-8, between two runs
    of trainer B itself), with every batch, pixel and parameter equal."""
    torch = gpu
    _, losses, _ = _reference(torch)
    got = _losses_of(torch, path)
    print(f"{path}: losses {got} vs trainer B {losses}; differences {[g - w for g, w in zip(got, losses)]}")
    assert got == losses


def test_checkpoint_keeps_the_place_in_the_sequence(gpu, tmp_path):
    torch = gpu
    import json
    import struct
    batches, losses, states = _reference(torch)
    a = _trainer(torch)
    a.step_images()
    a.step_images()
    path = str(tmp_path / "ck.rtxn")
    a.save_checkpoint(path)
    c = _trainer(torch)
    assert c.load_checkpoint(path)["draw_count"] == 2 and c.draw_count == 2 and int(c._draw_step.item()) == 2
    loss = float(c.step_images().item())
    assert torch.equal(c.drawn[:B], batches[2][3]) and np.isfinite(loss)
    _same(torch, c, states[2], "resumed")
    # attached after the load: the same place; a file without the key (written before device batches existed) starts at 0
    c2 = _trainer(torch, attach=False)
    c2.load_checkpoint(path)
    c2.attach_images(_set(torch)[0])
    assert c2.draw_count == 2 and int(c2._draw_step.item()) == 2
    raw = open(path, "rb").read()
    version, n = struct.unpack("<II", raw[8:16])
    header = json.loads(raw[16:16 + n])
    del header["draw_count"]
    blob = json.dumps(header).encode()
    blob += b" " * (n - len(blob))                              # same length: the arrays stay where they are
    old = str(tmp_path / "old.rtxn")
    open(old, "wb").write(raw[:16] + blob + raw[16 + n:])
    c.load_checkpoint(old)
    assert c.draw_count == 0 and int(c._draw_step.item()) == 0 and c.step_count == 2


def test_without_draw_an_attached_set_changes_nothing(gpu):
    """step() and capture_step() (draw left False) on a trainer WITH a set attached, fed trainer B's batches by hand: bit for bit
    trainer B, which has none -- and a captured trainer without a set alongside."""
    torch = gpu
    batches, losses, states = _reference(torch)
    x = _trainer(torch)
    for k in range(3):
        o, d, t, _ = batches[k]
        x.step(o, d, t)
        _same(torch, x, states[k], f"step() with a set attached, step {k}")
    assert x.draw_count == 0 and int(x._draw_step.item()) == 0
    y, z = _trainer(torch), _trainer(torch, attach=False)
    for tr in (y, z):
        tr.capture_step(B, launch_segments=B * 30)
    for k in range(3):
        o, d, t, _ = batches[k]
        for tr in (y, z):
            tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
            tr.step_captured()
        _same(torch, y, _state(z), f"captured, attached vs not, step {k}")
        _same(torch, y, states[k], f"step_captured() with a set attached, step {k}")
    assert y.draw_count == 0 and int(y._draw_step.item()) == 0
