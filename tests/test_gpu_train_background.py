"""Training over a background on the GPU: the compositor kernels against a float64 torch restatement and autograd,
the pinned per-ray hash of RANDOM backgrounds, bit-identity with the plain calls when no background is given, agreement of the
eager / captured / one-call steps, and end-to-end training on the sphere teacher over white and over random backgrounds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _fmix32(h):
    h = np.asarray(h, np.uint32)
    with np.errstate(over="ignore"):
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
        h = h ^ (h >> np.uint32(16))
    return h


def random_backgrounds(seed, step, n):
    """float32[n][3]: the RANDOM background of rays 0..n-1 (include/rtxn.h), restated in numpy"""
    with np.errstate(over="ignore"):
        h0 = _fmix32(np.uint32(seed) + np.uint32(0x9E3779B9) * np.uint32(step & 0xFFFFFFFF))
    r = np.arange(n, dtype=np.uint32)[:, None] * np.uint32(3) + np.arange(3, dtype=np.uint32)[None, :]
    h = _fmix32(h0 ^ r)
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _batch(rng, B, K):
    nh = rng.integers(0, 8, B).astype(np.int32)
    nh[::7] = 0                                       # rays without segments
    nh[3::50] = rng.integers(17, 40, nh[3::50].size)  # rays longer than 512 samples
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
    P = int(nh.sum())
    rad = np.concatenate([rng.uniform(0, 1, (P * K, 3)), rng.uniform(0, 1.5, (P * K, 1))], 1).astype(np.float32)
    step = rng.uniform(0.0, 0.2, P * K).astype(np.float32)
    return nh, idx, P, rad, step


def _reference(torch, rad, step, nh, K, bg, tgt):
    """float64: pixels = sum w c + (1 - A) bg, per-sample autograd-ready radiance"""
    B = nh.shape[0]
    ray = torch.from_numpy(np.repeat(np.arange(B), nh * K))
    c = torch.from_numpy(rad.astype(np.float64)).requires_grad_(True)
    d = torch.from_numpy(step.astype(np.float64))
    x = d * c[:, 3]
    cs = torch.cumsum(x, 0)
    start = torch.from_numpy(np.concatenate([[0], np.cumsum(nh * K)[:-1]]))
    off = torch.cat([torch.zeros(1, dtype=torch.float64), cs])[start][ray]       # sum of x before the ray's first sample
    T = torch.exp(-(cs - x - off))
    w = T * (1 - torch.exp(-x))
    col = torch.zeros((B, 3), dtype=torch.float64).index_add(0, ray, w[:, None] * c[:, :3])
    A = torch.zeros(B, dtype=torch.float64).index_add(0, ray, w)
    pix = col + (1 - A)[:, None] * torch.from_numpy(bg.astype(np.float64))
    return c, pix


def _composited(bg, tgt):
    """the target the kernel fits: RGBA composited over the background in fp32, as include/rtxn.h defines it"""
    if tgt.shape[1] == 3:
        return tgt.astype(np.float64)
    a = tgt[:, 3:4]
    return (a * tgt[:, :3] + (np.float32(1.0) - a) * bg).astype(np.float64)


@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("case", ["constant3", "constant4", "random4"])
def test_background_compositor_against_float64_autograd(gpu, K, case):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(K * 7 + len(case))
    B, ls = 777, 128.0
    nh, idx, P, rad, step = _batch(rng, B, K)
    tc = 3 if case == "constant3" else 4
    tgt = rng.uniform(0, 1, (B, tc)).astype(np.float32)
    if tc == 4:
        tgt[::5, 3] = 0.0
        tgt[1::5, 3] = 1.0
    if case.startswith("constant"):
        color = (0.9, 0.25, 1.0)
        bg_np = np.tile(np.array(color, np.float32), (B, 1))
        step_d = None
        bg = api.train_background(color, target_channels=tc)
    else:
        step_d = torch.full((1,), 41, dtype=torch.int32, device="cuda")
        bg_np = random_backgrounds(2024, 41, B)
        bg = api.train_background("random", seed=2024, step=step_d, target_channels=tc)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(rad=rad, step=step, nh=nh, idx=idx, tgt=tgt).items()}
    pix = torch.zeros((B, 3), device="cuda")
    lg = torch.zeros((B, 3), dtype=torch.float16, device="cuda")
    loss = torch.full((1,), 9.0, device="cuda")
    out = torch.zeros((P * K, 4), dtype=torch.float16, device="cuda")
    api.volrender_l2_train_ex(dev["rad"], dev["step"], dev["nh"], dev["idx"], B, K, dev["tgt"], ls, pix, lg, loss, out, bg)
    torch.cuda.synchronize()
    c, ref_pix = _reference(torch, rad, step, nh, K, bg_np, tgt)
    e = ref_pix.detach().numpy() - _composited(bg_np, tgt)
    got_pix = pix.cpu().numpy()
    pix_err = np.abs(got_pix - ref_pix.detach().numpy()).max()
    ref_loss = float((e ** 2).sum() / (3 * B))
    loss_err = abs(float(loss.item()) - ref_loss) / ref_loss
    want_lg = (ls * 2.0 * e / (3 * B)).astype(np.float16)
    lg_np = lg.cpu().numpy()
    lg_match = (lg_np.view(np.uint16) == want_lg.view(np.uint16)).mean()
    # radiance gradients: autograd of sum(pixel * g) with the kernel's own fp16 loss gradients
    (ref_pix * torch.from_numpy(lg_np.astype(np.float64))).sum().backward()
    want = c.grad.numpy()
    got = out.cpu().numpy().astype(np.float64)
    ratio = np.abs(got - want) / (1.5e-3 * np.abs(want) + 2e-5)
    print(f"\n[{case} K={K}] pixels max|err| {pix_err:.2e}  loss rel {loss_err:.2e}  fp16 loss grads equal {lg_match:.5f}  "
          f"radiance grads max|err| {np.abs(got - want).max():.2e}, max err / (1.5e-3 |want| + 2e-5) {ratio.max():.3f}")
    empty = nh == 0
    assert np.array_equal(got_pix[empty], bg_np[empty])                     # pixel = bg exactly
    # bars ~10x the errors measured on an MI355X (profiles/r06/train_background_ab.txt): pixels 2.5e-7, loss 2e-7 relative.
    # The radiance gradients keep test_gpu_train's bar: their error is the fp16 rounding of the output (2^-12 relative).
    np.testing.assert_allclose(got_pix, ref_pix.detach().numpy(), rtol=0, atol=3e-6)
    assert loss_err < 2e-6
    assert lg_match > 0.999
    np.testing.assert_allclose(got, want, rtol=1.5e-3, atol=2e-5)
    assert np.abs(want[:, 3]).max() > 1e-3 and np.abs(want[:, :3]).max() > 1e-3


@pytest.mark.parametrize("step", [0, 1, 12345])
def test_random_background_hash_is_pinned(gpu, step):
    torch = gpu
    from rtx_nerf_amd import api
    B, K, seed = 1000, 32, 0xDEADBEEF
    nh = np.zeros(B, np.int32)
    nh[::3] = 1
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
    P = int(nh.sum())
    rng = np.random.default_rng(step)
    rad = rng.uniform(0, 1, (P * K, 4)).astype(np.float32)
    st = rng.uniform(0, 0.1, P * K).astype(np.float32)
    tgt = rng.uniform(0, 1, (B, 4)).astype(np.float32)
    t = {k: torch.from_numpy(v).cuda() for k, v in dict(rad=rad, st=st, nh=nh, idx=idx, tgt=tgt).items()}
    step_d = torch.full((1,), step, dtype=torch.int32, device="cuda")
    pixels = []
    for s in (step, step + 1):
        step_d.fill_(s)
        pix = torch.zeros((B, 3), device="cuda")
        out = torch.zeros((P * K, 4), dtype=torch.float16, device="cuda")
        api.volrender_l2_train_ex(t["rad"], t["st"], t["nh"], t["idx"], B, K, t["tgt"], 1.0, pix, None, None, out,
                                  api.train_background("random", seed=seed, step=step_d, target_channels=4))
        pixels.append(pix.cpu().numpy())
    empty = nh == 0
    assert np.array_equal(pixels[0][empty].view(np.uint32), random_backgrounds(seed, step, B)[empty].view(np.uint32))
    assert np.array_equal(pixels[1][empty].view(np.uint32), random_backgrounds(seed, step + 1, B)[empty].view(np.uint32))
    assert (pixels[0][empty] != pixels[1][empty]).mean() > 0.99          # another step, other backgrounds
    assert 0.45 < pixels[0][empty].mean() < 0.55 and pixels[0][empty].min() >= 0 and pixels[0][empty].max() < 1


def test_no_background_is_the_plain_compositor_bit_for_bit(gpu):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(9)
    for K in (32, 7):
        B = 777
        nh, idx, P, rad, step = _batch(rng, B, K)
        tgt = rng.uniform(0, 1, (B, 3)).astype(np.float32)
        t = {k: torch.from_numpy(v).cuda() for k, v in dict(rad=rad, step=step, nh=nh, idx=idx, tgt=tgt).items()}
        res = []
        for bg in ("plain", None, api.train_background(None)):
            pix, lg = torch.zeros((B, 3), device="cuda"), torch.zeros((B, 3), dtype=torch.float16, device="cuda")
            out = torch.zeros((P * K, 4), dtype=torch.float16, device="cuda")
            if isinstance(bg, str):
                api.volrender_l2_train(t["rad"], t["step"], t["nh"], t["idx"], B, K, t["tgt"], 128.0, pix, lg, None, out)
            else:
                api.volrender_l2_train_ex(t["rad"], t["step"], t["nh"], t["idx"], B, K, t["tgt"], 128.0, pix, lg, None, out, bg)
            res.append((pix, lg, out))
        for r in res[1:]:
            for a, b in zip(res[0], r):
                assert torch.equal(a, b)


def _small_trainer(torch, encoding, seed=3, **kw):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer
    R, B = 16, 900
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()
    hgd = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
    return Trainer(R, occ, encoding=encoding, n_neurons=64, n_hidden_layers=4 if encoding == "hash" else 2,
                   hashgrid=hgd if encoding == "hash" else None, n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2,
                   loss_scale=128.0, density_scale=120.0, mode="nerf", seed=seed, **kw)


def _batches(torch, n, width, seed):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    focal = scenes.lego_focal_length(True)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        o, d = camera_rays(scenes.pose_spherical(25.0 + 55.0 * i, -28.0 + 4.0 * i, origin_scale=10.0), focal, 30, 30)
        t = rng.uniform(0, 1, (900, width)).astype(np.float32)
        if width == 4:
            t[::4, 3] = 0.0
        out.append((o, d, torch.from_numpy(t).cuda()))
    return out


def test_no_background_ex_calls_are_the_plain_calls_bit_for_bit(gpu):
    """RTXN_DETERMINISTIC: rtxn_train_gradients_ex(NULL) / rtxn_train_step_ex(NULL) leave exactly what the plain calls leave
    (pixels, loss gradients, radiance gradients, dparams, dtable, parameters); the loss sum to its float atomic's order."""
    torch = gpu
    from rtx_nerf_amd import api
    lib = api._lib.lib()
    (o, d, t), = _batches(torch, 1, 3, seed=2)
    for encoding in ("hash", "freq"):
        got = []
        for ex in (False, True):
            tr = _small_trainer(torch, encoding, deterministic=True)
            tr._det_select()
            tr._segments(o, d, 900)
            tr._clear_grads()
            hash_ = encoding == "hash"
            b = api.train_batch(tr.net, grid=tr.hg if hash_ else None, n_dir_freqs=tr.hg.n_dir_freqs if hash_ else 0,
                                table=tr.table if hash_ else None, start_points=tr.start, end_points=tr.end, seg_view=tr.seg_view,
                                num_stored=tr.num_stored, indices=tr.indices, total_segments=tr.total, segment_capacity=tr.max_segments,
                                n_rays=900, sample_type=tr._stype(), t_scale=tr.density_scale, vr_mode=api.VR_NERF, targets=t,
                                loss_scale=tr.loss_scale, encT=tr.encT, dencT=tr.dencT, workspace=tr.ws, output_half=tr.out,
                                radiance=tr.radiance, t_vals=tr.t_vals, radiance_gradients=tr.dout, pixels=tr.pixels,
                                loss_gradients=tr.loss_grads, loss_sum=tr.loss, dparams=tr.dparams,
                                dtable=tr.dtable if hash_ else None, dtable_hashed_half=tr.dtable_h if (hash_ and tr.hash_fp16) else None,
                                live_ws=tr.live_ws, workspace_lean=tr.lean)
            stream = api._stream()
            rc = lib.rtxn_train_gradients_ex(C.byref(b), None, stream) if ex else lib.rtxn_train_gradients(C.byref(b), stream)
            assert rc == 0
            torch.cuda.synchronize()
            S = int(tr.total.item()) * 32           # the radiance gradients past the batch's samples are never written
            got.append([x.clone() for x in (tr.pixels, tr.loss_grads, tr.dout[:S], tr.dparams, tr.table_grad() if hash_ else tr.dparams,
                                            tr.loss)])
        for a, b in zip(got[0][:-1], got[1][:-1]):
            assert torch.equal(a, b)
        assert abs(float(got[0][-1]) - float(got[1][-1])) <= 1e-6 * abs(float(got[0][-1]))
        # the one-call step
        got = []
        for ex in (False, True):
            tr = _small_trainer(torch, encoding, deterministic=True)
            tr._det_select()
            args = tr.entry_args(900, launch_segments=900 * 30)
            tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
            stream = api._stream()
            assert (lib.rtxn_train_step_ex(C.byref(args), None, stream) if ex else lib.rtxn_train_step(C.byref(args), stream)) == 0
            torch.cuda.synchronize()
            S = int(tr.total.item()) * 32
            got.append([x.clone() for x in (tr.pixels, tr.dout[:S], tr.master, tr.params, tr.entry_step)] +
                       ([tr.table_master.clone()] if encoding == "hash" else []))
        for a, b in zip(got[0], got[1]):
            assert torch.equal(a, b)


def test_plain_compositor_kernels_keep_their_machine_code(gpu):
    """the kernels of the plain training compositor (and the backward entry point) as built before background training existed"""
    import kernel_isa_hash
    want = {"volrender_l2_fused_multi_kernel": "f581d528df1205b7", "volrender_l2_fused_kernel": "d1bc313372473022",
            "volrender_bwd_nerf_kernel": "b8d436696adebe54", "volrender_bwd_compat_kernel": "2a13d105882c2ddc"}
    for k, h in want.items():
        assert kernel_isa_hash.kernel_isa_sha16([k]) == h, k


@pytest.mark.parametrize("encoding", ["hash", "freq"])
@pytest.mark.parametrize("background", [(1.0, 0.5, 0.0), "random"])
def test_eager_captured_and_one_call_steps_agree(gpu, encoding, background):
    """step(), step_captured() and step_entry() over the same background and batches: the same losses and parameters at the
    bars test_gpu_training_loop uses without a background (RANDOM: the same step numbers draw the same backgrounds on all
    three paths); then a captured step replayed twice on one batch draws new backgrounds."""
    torch = gpu
    width = 4 if background == "random" else 3
    kw = dict(background=background, background_seed=77)
    a, b, c = (_small_trainer(torch, encoding, **kw) for _ in range(3))
    batches = _batches(torch, 4, width, seed=8)
    b.capture_step(900, launch_segments=900 * 30)
    assert b.graph_targets.shape == (900, width)
    c.entry_args(900, launch_segments=900 * 30)
    for i, (o, d, t) in enumerate(batches):
        la = float(a.step(o, d, t).item())
        pa_pix = a.pixels.clone()
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        lb = float(b.step_captured().item())
        pb_pix = b.pixels.clone()
        c.graph_rays_o.copy_(o); c.graph_rays_d.copy_(d); c.graph_targets.copy_(t)
        lc = float(c.step_entry().item())
        assert abs(la - lb) <= 5e-4 * abs(la) and abs(la - lc) <= 5e-4 * abs(la), (i, la, lb, lc)
        empty = (a.num_stored[:900] == 0)
        assert int(empty.sum()) > 0
        assert torch.equal(pa_pix[empty], pb_pix[empty]) and torch.equal(pa_pix[empty], c.pixels[:900][empty])   # same backgrounds
    assert a.step_count == b.step_count == c.step_count == 4
    pa = a.master.cpu().numpy()
    for x in (b, c):
        assert np.linalg.norm(pa - x.master.cpu().numpy()) <= 3e-2 * np.linalg.norm(pa)
    o, d, t = batches[0]
    b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
    b.step_captured()
    p1 = b.pixels.clone()
    b.step_captured()
    p2 = b.pixels.clone()
    empty = b.num_stored[:900] == 0
    if background == "random":
        assert (p1[empty] != p2[empty]).float().mean() > 0.99
    else:
        assert torch.equal(p1[empty], p2[empty])


def test_training_over_white_and_random_backgrounds(gpu):
    """The sphere teacher, trained over white (targets composited over white) and over random backgrounds (RGBA targets).
    White: held-out PSNR over white rises by a clear margin.  Random: held-out PSNR over white AND over black each come
    within a few dB of the white-trained model's over white -- the opacity is learned, not baked into the colour."""
    import train_demo
    w0, w1, wl = train_demo.run(steps=300, encoding="hash", background=(1.0, 1.0, 1.0), verbose=False)
    r0, r1, rl = train_demo.run(steps=300, encoding="hash", background="random", rgba=True, verbose=False)
    print(f"\nwhite-trained: {w0} -> {w1}\nrandom-trained: {r0} -> {r1}")
    assert wl[-1] < 0.1 * wl[0], wl
    assert w1["white"] > w0["white"] + 4.5, (w0, w1)      # measured: +6.9 dB (15.3 -> 22.2)
    # measured: 26.0 dB over white, 26.1 over black (the white-trained model: 22.2 over white)
    assert r1["white"] > w1["white"] - 3.0 and r1["black"] > w1["white"] - 3.0, (w1, r1)
