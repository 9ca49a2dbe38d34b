"""End-to-end training on the GPU: the loss falls and held-out PSNR rises when the
hash-grid / frequency models are fitted to an analytic teacher field through the full
stage chain (trace -> sample -> encode -> MLP fwd -> composite -> L2 -> composite bwd ->
MLP bwd -> hash scatter -> Adam)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.mark.parametrize("encoding,steps,gain", [("hash", 300, 7.0), ("freq", 300, 5.0)])
def test_training_converges(gpu, encoding, steps, gain):
    import train_demo
    p0, p1, losses = train_demo.run(steps=steps, encoding=encoding, grid=32, res=64, batch=4096, n_poses=12, verbose=False)
    assert losses[-1] < 0.1 * losses[0], losses
    assert p1 > p0 + gain, (p0, p1)          # held-out pose, measured: hash +10.5 dB, freq +7.7 dB


TODAY = dict(n_levels=4, n_features=2, log2_hashmap_size=11, base_resolution=4, per_level_scale=1.6)
# The same step on the grids the Trainer had never seen (tests/test_gpu_hashgrid_float64.py holds the kernels themselves to
# float64): four features (fp32 scatter, general encoder), one feature with an odd level count, every level hashed
# (hashed_offset() == 0: empty dense slices into Adam) and every level dense (hashed_offset() == n_params: no fp16 gradient).
OTHER_GRIDS = {
    "f4": dict(TODAY, n_features=4),
    "f1-odd": dict(TODAY, n_levels=5, n_features=1),
    "all-hashed": dict(n_levels=4, n_features=2, log2_hashmap_size=8, base_resolution=16, per_level_scale=1.6),
    "all-dense": dict(n_levels=3, n_features=2, log2_hashmap_size=19, base_resolution=4, per_level_scale=1.6),
}


def test_config3_training_step_matches_oracle_chain(gpu, oracle):
    """BASELINE configs[2] in miniature (hash-grid encoding + 4x64 MLP, one ray batch): every stage of one
    optimisation step on the GPU against the same step chained from oracle functions."""
    _config3_step(gpu, oracle, TODAY)


@pytest.mark.parametrize("grid", list(OTHER_GRIDS))
def test_config3_training_step_matches_oracle_chain_on_other_grids(gpu, oracle, grid):
    hgd = OTHER_GRIDS[grid]
    tr = _config3_step(gpu, oracle, hgd)
    n = tr.hg.n_params()
    if grid in ("all-hashed", "all-dense"):
        assert tr.hashed_lo == (0 if grid == "all-hashed" else n)
    else:
        assert 0 < tr.hashed_lo < n
    assert tr.hash_fp16 == (hgd["n_features"] == 2 and tr.hashed_lo < n)


def _config3_step(gpu, oracle, hgd):
    import numpy as np
    torch = gpu
    from rtx_nerf_amd import api, scenes
    from rtx_nerf_amd.train import Trainer, camera_rays
    R, B, scale, ls = 16, 900, 120.0, 128.0
    dense = scenes.sphere_density(R, 0.75)
    words = scenes.pack_occupancy(dense)
    occ = torch.from_numpy(words.view(np.int32).copy()).cuda()
    tr = Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=4, hashgrid=hgd, n_dir_freqs=4, batch_rays=B,
                 max_segments=B * 30, lr=1e-2, loss_scale=ls, density_scale=scale, mode="nerf", seed=3)
    # give the table non-trivial values so the encoding is not ~0
    g = torch.Generator().manual_seed(5)
    tr.table_master.copy_(((torch.rand(tr.hg.n_params(), generator=g) * 2 - 1) * 0.5).cuda())
    tr.table.copy_(tr.table_master.half())
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
    rng = np.random.default_rng(0)
    tgt = torch.from_numpy(rng.uniform(0, 1, (B, 3)).astype(np.float32)).cuda()
    params0 = tr.params.cpu().numpy().copy()
    table0 = tr.table.cpu().numpy().copy()
    master0, tmaster0 = tr.master.cpu().numpy().copy(), tr.table_master.cpu().numpy().copy()
    loss = float(tr.step(o, d, tgt).item())
    P = int(tr.total.item())
    S = P * 32
    t_folded = tr.t_vals[:S].clone()      # written by the encoder (sampler folded in)
    tr.materialize_samples(B)             # the standalone sampler over the same segments, for the comparison below
    assert torch.equal(tr.t_vals[:S], t_folded)

    # ---- the same step from oracle pieces -------------------------------------------------------
    O = oracle
    on, dn = o.cpu().numpy(), d.cpu().numpy()
    pk = O.trace_packed(rays_o=on, rays_d=dn, R=R, occ=words, mode=1)
    assert pk["total"] == P
    samples, steps = O.sample(pk["start"], pk["end"], pk["view_dirs"], pk["num_hits"], pk["indices"], 3)
    np.testing.assert_array_equal(tr.samples[:S].cpu().numpy()[:, :3], samples[:, :3])
    steps = steps * np.float32(scale)
    ocfg = O.hg_cfg(**hgd)
    # view angles come from the device's atan2f; use the GPU's own (theta, phi) so the encodings are comparable
    samples[:, 3:] = tr.samples[:S].cpu().numpy()[:, 3:]
    enc = O.encode_hg(ocfg, 4, table0, samples)
    acts, out = O.mlpe_forward(64, 4, 1, params0, enc)
    rad = out[:, :4].astype(np.float32)
    pix = O.volrender_fwd_nerf(rad, pk["num_hits"], pk["indices"], steps)
    np.testing.assert_allclose(tr.pixels.cpu().numpy(), pix, rtol=0, atol=3e-3)
    o_loss, _, g16, _ = O.l2_loss(pix, tgt.cpu().numpy(), ls)
    assert abs(loss - o_loss) < 2e-3 * o_loss
    # continue the oracle chain from the GPU's forward state (radiance, loss gradients) so that the backward
    # comparison is not dominated by forward rounding differences
    rad_g = tr.radiance[:S].cpu().numpy()
    lg = tr.loss_grads.cpu().numpy()
    dout = O.volrender_bwd_nerf(lg, rad_g, steps, pk["num_hits"], pk["indices"]).astype(np.float16)
    np.testing.assert_allclose(tr.dout[:S].cpu().numpy().astype(np.float32), dout.astype(np.float32), rtol=2e-3, atol=1e-6)
    Sp = api.padded_samples(S)
    enc_g = tr.encT.reshape(-1)[:tr.E * Sp].reshape(tr.E, Sp)[:, :S].t().contiguous().cpu().numpy()
    if tr.recompute:    # the fused backward rebuilds the activations on the chip and never stores them: the oracle's own, from the GPU's encoding
        acts_g, _ = O.mlpe_forward(64, 4, 1, params0, enc_g)
    else:
        acts_g = tr.ws[:4 * 64 * Sp].reshape(4, 64, Sp)[:, :, :S].permute(0, 2, 1).contiguous().cpu().numpy()
    dp, denc = O.mlpe_backward(64, 4, 1, params0, enc_g, acts_g, tr.out[:S].cpu().numpy(), tr.dout[:S].cpu().numpy())
    got_dp = tr.dparams.cpu().numpy()
    assert np.linalg.norm(got_dp - dp) < 2e-2 * np.linalg.norm(dp) and np.abs(dp).max() > 0
    denc_g = tr.dencT.reshape(-1)[:tr.E * Sp].reshape(tr.E, Sp)[:, :S].t().contiguous().cpu().numpy()
    if tr.live_segments:
        # the backward visited only the segments with a loss gradient (rtxn_live_segments): d(encoding) of the others was never
        # written and nothing reads it -- for the oracle, which walks every sample, those columns are the zeros they stand for
        n_live = int(tr.live_ws[0].item())
        listed = tr.live_ws[4:4 + n_live].cpu().numpy()
        want_live = np.nonzero((tr.dout[:S].cpu().numpy().reshape(P, 32, 4).view(np.uint16) & 0x7fff).any(axis=(1, 2)))[0]
        np.testing.assert_array_equal(listed, want_live)
        assert 0 < n_live < P
        dead = np.ones(P, bool)
        dead[listed] = False
        assert np.abs(denc[np.repeat(dead, 32)]).max() == 0.0          # and the oracle agrees that they are zero
        denc_g[np.repeat(dead, 32)] = 0
    dt = O.hg_backward(ocfg, samples, denc_g)
    got_dt = tr.table_grad().cpu().numpy()
    # hashed levels are accumulated in fp16 (packed atomics): 11-bit contributions
    assert np.abs(got_dt - dt).max() < (1e-2 if tr.hash_fp16 else 1e-3) * max(1e-6, np.abs(dt).max())   # fp16 atomics: order-dependent
    assert np.linalg.norm(got_dt - dt) < (2e-3 if tr.hash_fp16 else 1e-3) * np.linalg.norm(dt)
    # Adam from the GPU's gradients reproduces the GPU's new parameters
    m, v = np.zeros_like(master0), np.zeros_like(master0)
    O.adam_step(master0, got_dp, m, v, 1, lr=1e-2, loss_scale=ls)
    np.testing.assert_allclose(tr.master.cpu().numpy(), master0, rtol=0, atol=2e-6)
    m, v = np.zeros_like(tmaster0), np.zeros_like(tmaster0)
    steps = np.zeros(tmaster0.size, np.uint32)           # the table: tiny-cuda-nn's non-matrix rule (zero gradient -> untouched)
    O.adam_step_sparse(tmaster0, got_dt, m, v, steps, lr=1e-1, eps=1e-15, loss_scale=ls)
    np.testing.assert_allclose(tr.table_master.cpu().numpy(), tmaster0, rtol=0, atol=2e-6)
    np.testing.assert_array_equal(tr.table_steps.cpu().numpy().view(np.uint32), steps)
    assert 0 < int(steps.sum()) < steps.size
    return tr


def test_compat_training_step_matches_oracle_chain(gpu, oracle):
    """The reference's OWN training iteration (main.cu:704-787) end to end, Trainer(mode="compat"): REGULAR sampler ->
    Composite-Frequency encoding + 128-wide ReLU MLP forward -> COMPAT composite (vol_render.cu:19-73) -> L2 -> COMPAT
    backward (vol_render.cu:75-143, literally: not the gradient of the forward) -> network backward -> Adam, every
    stage against the same step chained from oracle functions."""
    import numpy as np
    torch = gpu
    from rtx_nerf_amd import api, scenes
    from rtx_nerf_amd.train import Trainer, camera_rays
    R, ls, W, L = 16, 128.0, 128, 3
    dense = scenes.sphere_density(R, 0.75)
    words = scenes.pack_occupancy(dense)
    occ = torch.from_numpy(words.view(np.int32).copy()).cuda()
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 24, 24)
    B = o.shape[0]
    tr = Trainer(R, occ, encoding="freq", n_neurons=W, n_hidden_layers=L, n_dir_freqs=12, batch_rays=B,
                 max_segments=B * 30, lr=1e-3, loss_scale=ls, mode="compat", seed=3)
    rng = np.random.default_rng(0)
    tgt = torch.from_numpy(rng.uniform(0, 1, (B, 3)).astype(np.float32)).cuda()
    params0, master0 = tr.params.cpu().numpy().copy(), tr.master.cpu().numpy().copy()
    loss = float(tr.step(o, d, tgt).item())
    P = int(tr.total.item())
    S = P * 32
    assert S > 20_000 and tr.step_count == 1
    t_folded = tr.t_vals[:S].clone()
    tr.materialize_samples(B)
    assert torch.equal(tr.t_vals[:S], t_folded)

    O = oracle
    pk = O.trace_packed(rays_o=o.cpu().numpy(), rays_d=d.cpu().numpy(), R=R, occ=words, mode=1)
    assert pk["total"] == P
    samples, t_vals = O.sample(pk["start"], pk["end"], pk["view_dirs"], pk["num_hits"], pk["indices"], 0)   # SAMPLING_REGULAR
    np.testing.assert_array_equal(tr.samples[:S].cpu().numpy()[:, :3], samples[:, :3])
    np.testing.assert_array_equal(tr.t_vals[:S].cpu().numpy(), t_vals)
    samples[:, 3:] = tr.samples[:S].cpu().numpy()[:, 3:]       # (theta, phi): the device's atan2f (2e-6 from glibc's)
    cfg = O.mlp_cfg(n_neurons=W, n_hidden_layers=L)
    enc = O.encode_freq(cfg, samples)
    acts, out = O.mlpe_forward(W, L, 1, params0, enc)
    rad = out[:, :4].astype(np.float32)
    np.testing.assert_allclose(tr.radiance[:S].cpu().numpy(), rad, rtol=0, atol=1e-2)
    pix = O.volrender_fwd(rad, pk["num_hits"], pk["indices"], t_vals)
    np.testing.assert_allclose(tr.pixels.cpu().numpy(), pix, rtol=0, atol=3e-3)
    o_loss, _, _, _ = O.l2_loss(pix, tgt.cpu().numpy(), ls)
    assert abs(loss - o_loss) < 5e-3 * o_loss
    # backward from the GPU's own forward state, so that the comparison is not dominated by forward rounding
    rad_g, lg = tr.radiance[:S].cpu().numpy(), tr.loss_grads.cpu().numpy()
    dout = O.volrender_bwd(lg, rad_g, t_vals, pk["num_hits"], pk["indices"])
    got_dout = tr.dout[:S].cpu().numpy()
    assert (got_dout.view(np.uint16) == np.asarray(dout, np.float16).view(np.uint16)).mean() > 0.995   # <= 1 fp16 ulp elsewhere
    Sp = api.padded_samples(S)
    acts_g = tr.ws[:L * W * Sp].reshape(L, W, Sp)[:, :, :S].permute(0, 2, 1).contiguous().cpu().numpy()
    enc_g = tr.encT.reshape(-1)[:tr.E * Sp].reshape(tr.E, Sp)[:, :S].t().contiguous().cpu().numpy()
    assert np.abs(enc_g.astype(np.float32) - enc.astype(np.float32)).max() < 2e-3
    dp, _ = O.mlpe_backward(W, L, 1, params0, enc_g, acts_g, tr.out[:S].cpu().numpy(), got_dout, want_denc=False)
    got_dp = tr.dparams.cpu().numpy()
    assert np.abs(dp).max() > 0 and np.linalg.norm(got_dp - dp) < 2e-2 * np.linalg.norm(dp)
    m, v = np.zeros_like(master0), np.zeros_like(master0)
    O.adam_step(master0, got_dp, m, v, 1, lr=1e-3, loss_scale=ls)
    np.testing.assert_allclose(tr.master.cpu().numpy(), master0, rtol=0, atol=2e-6)


def _small_trainer(torch, encoding, mode, neurons, layers, seed=3, hgd=None, **kw):
    import numpy as np
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer
    R, B = 16, 900
    words = scenes.pack_occupancy(scenes.sphere_density(R, 0.75))
    occ = torch.from_numpy(words.view(np.int32).copy()).cuda()
    hgd = hgd or TODAY
    return Trainer(R, occ, encoding=encoding, n_neurons=neurons, n_hidden_layers=layers, hashgrid=hgd if encoding == "hash" else None,
                   n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2, loss_scale=128.0,
                   density_scale=120.0 if mode == "nerf" else 1.0, mode=mode, seed=seed, **kw)


@pytest.mark.parametrize("encoding,mode,neurons,layers", [("hash", "nerf", 64, 4), ("freq", "nerf", 128, 2), ("freq", "compat", 64, 2),
                                                          ("hash", "compat", 128, 2)])
def test_captured_step_matches_the_eager_step(gpu, encoding, mode, neurons, layers):
    _captured_vs_eager(gpu, encoding, mode, neurons, layers)


@pytest.mark.parametrize("grid", ["f4", "all-hashed"])
def test_captured_step_matches_the_eager_step_on_other_grids(gpu, grid):
    _captured_vs_eager(gpu, "hash", "nerf", 64, 4, hgd=OTHER_GRIDS[grid])


def _captured_vs_eager(gpu, encoding, mode, neurons, layers, hgd=None):
    """Trainer.capture_step / step_captured (one hipGraph: traversal -> rtxn_train_gradients with the segment count read on the
    device -> Adam -> re-pack) against Trainer.step (per-stage entry points, segment count on the host) on the same batches:
    same loss and the same parameters after several steps, up to the order of the fp32 / fp16 atomics.  Covers the recompute
    path (64 x 4 hash), the saved-activation path with its weight-gradient GEMM (128 wide) and both compositor modes; the graph
    is sized for MORE segments than any batch has, so every kernel runs with blocks past the live samples."""
    import numpy as np
    torch = gpu
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    a = _small_trainer(torch, encoding, mode, neurons, layers, hgd=hgd)
    b = _small_trainer(torch, encoding, mode, neurons, layers, hgd=hgd)
    B = 900
    focal = scenes.lego_focal_length(True)
    rng = np.random.default_rng(1)
    batches = []
    for i in range(6):
        o, d = camera_rays(scenes.pose_spherical(40.0 + 50.0 * i, -30.0 + 5.0 * i, origin_scale=10.0), focal, 30, 30)
        batches.append((o, d, torch.from_numpy(rng.uniform(0, 1, (B, 3)).astype(np.float32)).cuda()))
    b.capture_step(B, launch_segments=B * 30)
    assert torch.equal(a.params, b.params) and b.step_count == 0          # the warm-up pass of the capture left no trace
    for i, (o, d, t) in enumerate(batches):
        la = float(a.step(o, d, t).item())
        P = int(a.total.item())
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        lb = float(b.step_captured().item())
        assert int(b.total.item()) == P and 0 < P < B * 30
        assert abs(la - lb) <= 5e-4 * abs(la), (i, la, lb)
        if i == 0:
            # same parameters going in.  The captured optimizer clears every gradient as it consumes it (nothing to compare
            # there: they must read zero), so the first step is compared through the parameters it produced: Adam at step 1
            # moves every weight by ~lr * sign(g), which is compared where the gradient is not noise
            ga = a.dparams.cpu().numpy()
            assert np.linalg.norm(ga) > 0 and float(b.dparams.abs().max()) == 0.0
            if encoding == "hash":
                assert float(b.table_grad().abs().max()) == 0.0
            big = np.abs(ga) > 1e-3 * np.abs(ga).max()
            pa, pb = a.master.cpu().numpy(), b.master.cpu().numpy()
            np.testing.assert_allclose(pa[big], pb[big], rtol=0, atol=2e-4)
            if encoding == "hash":
                ta, tb = a.table_master.cpu().numpy(), b.table_master.cpu().numpy()
                tg = a.table_grad().cpu().numpy()
                tbig = np.abs(tg) > 1e-2 * np.abs(tg).max()
                np.testing.assert_allclose(ta[tbig], tb[tbig], rtol=0, atol=2e-3)
    assert a.step_count == b.step_count == 6 and b.truncated_steps == 0
    pa, pb = a.master.cpu().numpy(), b.master.cpu().numpy()
    assert np.linalg.norm(pa - pb) <= 3e-2 * np.linalg.norm(pa)          # six Adam steps at lr 1e-2 amplify gradient noise


@pytest.mark.parametrize("encoding,mode,neurons,layers", [("hash", "nerf", 64, 4), ("freq", "compat", 128, 2), ("freq", "nerf", 128, 3)])
def test_train_step_entry_matches_the_eager_step(gpu, encoding, mode, neurons, layers):
    _entry_vs_eager(gpu, encoding, mode, neurons, layers)


@pytest.mark.parametrize("grid", ["f4", "all-hashed"])
def test_train_step_entry_matches_the_eager_step_on_other_grids(gpu, grid):
    _entry_vs_eager(gpu, "hash", "nerf", 64, 4, hgd=OTHER_GRIDS[grid])


def _entry_vs_eager(gpu, encoding, mode, neurons, layers, hgd=None):
    """rtxn_train_step -- traversal, rtxn_train_gradients, tiny-cuda-nn's Adam (device step counter) and the weight re-pack of one
    batch as ONE C call, what a C++ host uses (examples/train_host.cpp) -- against Trainer.step (per-stage entry points, host
    step count) on the same batches: same losses, same parameters up to the order of the atomics; then the same call captured
    into a hipGraph and replayed."""
    import numpy as np
    torch = gpu
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    a = _small_trainer(torch, encoding, mode, neurons, layers, hgd=hgd)
    b = _small_trainer(torch, encoding, mode, neurons, layers, hgd=hgd)
    a_table0 = a.table_master.cpu().numpy().copy() if encoding == "hash" else None
    B = 900
    focal = scenes.lego_focal_length(True)
    rng = np.random.default_rng(5)
    batches = []
    for i in range(6):
        o, d = camera_rays(scenes.pose_spherical(25.0 + 55.0 * i, -28.0 + 4.0 * i, origin_scale=10.0), focal, 30, 30)
        batches.append((o, d, torch.from_numpy(rng.uniform(0, 1, (B, 3)).astype(np.float32)).cuda()))
    b.entry_args(B, launch_segments=B * 30)
    for i, (o, d, t) in enumerate(batches[:4]):
        la = float(a.step(o, d, t).item())
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        lb = float(b.step_entry().item())
        assert int(b.total.item()) == int(a.total.item()) > 0
        assert abs(la - lb) <= 5e-4 * abs(la), (i, la, lb)
        assert int(b.entry_step.item()) == i + 1 == b.step_count
        assert float(b.dparams.abs().max()) == 0.0           # consumed and cleared
    # the rest of the batches through a captured graph of the same call
    from rtx_nerf_amd import api
    g = torch.cuda.CUDAGraph()
    state = [x.clone() for x in (b.master, b.params, b.adam_m, b.adam_v, b.entry_step)]
    tstate = [x.clone() for x in (b.table_master, b.table, b.table_m, b.table_v, b.table_steps)] if encoding == "hash" else []
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        api.train_step(b._entry_args)
    torch.cuda.synchronize()
    # (capturing does not execute: nothing to undo)
    for x, y in zip((b.master, b.params, b.adam_m, b.adam_v, b.entry_step), state):
        assert torch.equal(x, y)
    for x, y in zip((b.table_master, b.table, b.table_m, b.table_v, b.table_steps) if encoding == "hash" else (), tstate):
        assert torch.equal(x, y)
    for i, (o, d, t) in enumerate(batches[4:]):
        la = float(a.step(o, d, t).item())
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        g.replay()
        lb = float(b.loss.item())
        assert abs(la - lb) <= 1e-3 * abs(la), (i, la, lb)
    assert int(b.entry_step.item()) == 6
    pa, pb = a.master.cpu().numpy(), b.master.cpu().numpy()
    assert np.linalg.norm(pa - pb) <= 3e-2 * np.linalg.norm(pa)
    if encoding == "hash":
        # The table's gradient is summed by fp16 atomics in an order that changes from run to run, and Adam turns an ulp of a
        # near-zero gradient into a whole +-lr step: two IDENTICAL eager trainers on these batches end 0.014-0.067 apart in
        # relative norm (12 runs on the GPU), with 5-19 % of the moved entries differing by more than 1e-3.  The bar is what
        # separates that from a wrong optimiser path (a missed step, wrong step counts: relative distance of order 1).
        ta, tb = a.table_master.cpu().numpy(), b.table_master.cpu().numpy()
        assert np.linalg.norm(ta - tb) <= 0.2 * np.linalg.norm(ta)
        moved = (ta != a_table0) | (tb != a_table0)
        assert moved.sum() > 1000 and (np.abs(ta - tb)[moved] <= 1e-3).mean() >= 0.6


def test_captured_step_with_the_traversal_one_batch_ahead(gpu):
    """capture_step(prefetch=True): every step_captured() call traverses the batch it is given as a parallel branch beside the
    gradient kernels of the batch given to the previous call.  Same losses as the eager step, one call later; flush_captured()
    trains on the last batch; two buffer sets alternate (an odd and an even number of steps are both exercised)."""
    import numpy as np
    torch = gpu
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    a = _small_trainer(torch, "hash", "nerf", 64, 4)
    b = _small_trainer(torch, "hash", "nerf", 64, 4)
    B = 900
    focal = scenes.lego_focal_length(True)
    rng = np.random.default_rng(2)
    batches = []
    for i in range(5):
        o, d = camera_rays(scenes.pose_spherical(10.0 + 70.0 * i, -25.0 - 4.0 * i, origin_scale=10.0), focal, 30, 30)
        batches.append((o, d, torch.from_numpy(rng.uniform(0, 1, (B, 3)).astype(np.float32)).cuda()))
    b.capture_step(B, launch_segments=B * 20, prefetch=True)
    eager = [float(a.step(o, d, t).item()) for o, d, t in batches]
    got = []
    for o, d, t in batches:
        b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
        r = b.step_captured()
        got.append(None if r is None else float(r.item()))
    assert got[0] is None and b.step_count == 4
    got = got[1:] + [float(b.flush_captured().item())]
    assert b.step_count == 5 and b.flush_captured() is None and b.truncated_steps == 0
    for i, (x, y) in enumerate(zip(eager, got)):
        assert abs(x - y) <= 1e-3 * abs(x), (i, eager, got)
    pa, pb = a.master.cpu().numpy(), b.master.cpu().numpy()
    assert np.linalg.norm(pa - pb) <= 3e-2 * np.linalg.norm(pa)
    # and on: a new batch after the flush primes again
    o, d, t = batches[0]
    b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
    assert b.step_captured() is None
    assert np.isfinite(float(b.flush_captured().item())) and b.step_count == 6


def test_captured_step_truncates_on_the_device_and_reports_it(gpu):
    """A graph sized for fewer segments than the batch needs: rays are cut off by the traversal (num_stored), nothing is
    written out of bounds, the step still runs, and the next call reports the truncation."""
    import warnings
    import numpy as np
    torch = gpu
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    tr = _small_trainer(torch, "hash", "nerf", 64, 4)
    B = 900
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
    t = torch.full((B, 3), 0.5, device="cuda")
    tr.step(o, d, t)
    need = int(tr.total.item())
    cap = need // 2
    guard = tr.start.clone()
    tr.capture_step(B, launch_segments=cap)
    tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
    tr.step_captured()
    torch.cuda.synchronize()
    assert int(tr.num_stored[:B].sum().item()) <= cap < int(tr.num_hits[:B].sum().item())
    assert np.isfinite(float(tr.loss.item()))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tr.step_captured()
    assert tr.truncated_steps == 1 and any("truncated" in str(x.message) for x in w)
    assert torch.equal(tr.start[cap:], guard[cap:])        # nothing stored past the launch capacity


def test_captured_step_on_a_batch_that_misses_the_grid(gpu):
    """Every ray misses the occupied cells: the device-side segment count is 0, every kernel of the captured step must leave at
    once (no tile, no live segment, no atomics), the loss is the mean squared target, and Adam on an all-zero gradient with
    zero moments leaves the parameters where they were.  Then a normal batch trains as usual (nothing was left in a bad state)."""
    import numpy as np
    torch = gpu
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    tr = _small_trainer(torch, "hash", "nerf", 64, 4)
    B = 900
    tr.capture_step(B, launch_segments=B * 20)
    p0, t0 = tr.master.clone(), tr.table_master.clone()
    tr.graph_rays_o.copy_(torch.tensor([5.0, 5.0, 5.0], device="cuda").repeat(B, 1))
    tr.graph_rays_d.copy_(torch.tensor([0.0, 0.0, 1.0], device="cuda").repeat(B, 1))      # pointing away from [-1,1]^3
    tgt = torch.full((B, 3), 0.5, device="cuda")
    tr.graph_targets.copy_(tgt)
    loss = float(tr.step_captured().item())
    torch.cuda.synchronize()
    assert int(tr.total.item()) == 0 and abs(loss - 0.25) < 1e-6
    assert torch.equal(tr.master, p0) and torch.equal(tr.table_master, t0)
    assert int(tr.live_ws[0].item()) == 0
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
    tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d)
    l1 = float(tr.step_captured().item())
    for _ in range(20):
        l2 = float(tr.step_captured().item())
    assert int(tr.total.item()) > 0 and np.isfinite(l2) and l2 < l1 and not torch.equal(tr.master, p0)


def test_captured_step_sees_an_occupancy_refresh(gpu):
    """capture_step() bakes the device pointers of the occupancy hierarchy into the traversal nodes; a refresh must
    write into THOSE buffers (Trainer._set_occupancy) -- re-binding the attributes left the graphs traversing freed memory.
    capture, empty the grid (threshold 1e9), replay: no ray may hit anything; fill it (threshold -1), replay: every ray that
    enters the cube hits."""
    torch = gpu
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    tr = _small_trainer(torch, "hash", "nerf", 64, 4)
    B = 900
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
    tr.capture_step(B, launch_segments=B * 30)
    tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.fill_(0.5)
    tr.step_captured()
    torch.cuda.synchronize()
    before = int(tr.total.item())
    ptrs = [t.data_ptr() for t in (tr.occ, tr.coarse, tr.bricks, tr.super_mip)]
    assert before > 0
    assert tr.update_occupancy(threshold=1e9) == 0.0
    assert ptrs == [t.data_ptr() for t in (tr.occ, tr.coarse, tr.bricks, tr.super_mip)] and tr._graphs is not None
    tr.step_captured()
    torch.cuda.synchronize()
    assert int(tr.total.item()) == 0
    assert tr.update_occupancy(threshold=-1.0) == 1.0
    tr.step_captured()
    torch.cuda.synchronize()
    assert int(tr.total.item()) > before


def test_captured_adam_follows_the_host_step_count(gpu):
    """the captured Adam reads its bias-corrected rate through a DEVICE step counter that only replays advance.  An
    eager step() in between (supported) and load_checkpoint() move step_count on the host only; the next replay must use
    the rate of step_count + 1 all the same: eager-only and mixed eager/captured runs end at the same parameters."""
    import numpy as np
    torch = gpu
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    a = _small_trainer(torch, "freq", "nerf", 64, 2)
    b = _small_trainer(torch, "freq", "nerf", 64, 2)
    B = 900
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
    t = torch.full((B, 3), 0.5, device="cuda")
    b.capture_step(B, launch_segments=B * 30)
    b.graph_rays_o.copy_(o); b.graph_rays_d.copy_(d); b.graph_targets.copy_(t)
    for kind in ("eager", "eager", "eager", "captured", "eager", "captured"):   # the rate changes fastest in the first steps
        a.step(o, d, t)
        if kind == "eager":
            b.step(o, d, t)
        else:
            b.step_captured()
    torch.cuda.synchronize()
    assert a.step_count == b.step_count == 6 and int(b._g_step.item()) == 6
    pa, pb = a.master.cpu().numpy(), b.master.cpu().numpy()
    assert np.linalg.norm(pa - pb) <= 2e-3 * np.linalg.norm(pa), np.linalg.norm(pa - pb) / np.linalg.norm(pa)


def _det_batches(torch, n=6, B=900):
    import numpy as np
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    focal = scenes.lego_focal_length(True)
    rng = np.random.default_rng(5)
    out = []
    for i in range(n):
        o, d = camera_rays(scenes.pose_spherical(25.0 + 55.0 * i, -28.0 + 4.0 * i, origin_scale=10.0), focal, 30, 30)
        out.append((o, d, torch.from_numpy(rng.uniform(0, 1, (B, 3)).astype(np.float32)).cuda()))
    return out


def _state(tr):
    import torch
    s = [tr.master, tr.params, tr.adam_m, tr.adam_v]
    if tr.encoding == "hash":
        s += [tr.table_master, tr.table, tr.table_m, tr.table_v, tr.table_steps]
    return [x.clone() for x in s]


@pytest.mark.parametrize("encoding,mode,neurons,layers", [("hash", "nerf", 64, 4), ("hash", "compat", 128, 2), ("freq", "nerf", 128, 8),
                                                          ("freq", "compat", 128, 8), ("freq", "nerf", 64, 2)])
def test_deterministic_mode_makes_two_trainers_bit_identical(gpu, encoding, mode, neurons, layers):
    """VERDICT r03 item 4 / missing 4: Trainer(deterministic=True) -- every cross-workgroup gradient sum in 64-bit fixed point
    (rtxn_set_deterministic_workspace) instead of float atomics.  Two trainers fed the same batches must then hold IDENTICAL
    parameters, optimizer state and hash table after six Adam steps, bit for bit -- the eager step against itself, and the eager
    step against rtxn_train_step (one C call per step) -- where the default mode needs the tolerances of the tests above
    (0.2 in relative norm on the table).  Covers the fused 64-wide backward + hash scatter, the saved-activation weight-gradient
    kernels (128 x 2) and the lean 8 x 128 path; run again, a third trainer reproduces the first."""
    import numpy as np
    torch = gpu
    batches = _det_batches(torch)
    a = _small_trainer(torch, encoding, mode, neurons, layers, deterministic=True)
    b = _small_trainer(torch, encoding, mode, neurons, layers, deterministic=True)
    c = _small_trainer(torch, encoding, mode, neurons, layers, deterministic=True)
    assert a.deterministic and a._det_mlp is not None and (a._det_table is not None) == (encoding == "hash")
    B = batches[0][0].shape[0]
    c.entry_args(B, launch_segments=B * 30)
    for i, (o, d, t) in enumerate(batches):
        la = a.step(o, d, t).clone()
        lb = b.step(o, d, t).clone()
        c.graph_rays_o.copy_(o); c.graph_rays_d.copy_(d); c.graph_targets.copy_(t)
        c.step_entry()
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(_state(a), _state(b))):
            assert torch.equal(x, y), f"eager vs eager: step {i}, tensor {k}: {int((x != y).sum())} of {x.numel()} differ"
        assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(la))      # (the reported loss sum stays a float atomic)
        if i == 0:
            # one step: the same gradients bit for bit, Adam's beta^t from the device counter (v_exp_f32) against the host's: measured
            # 0 to 7e-8 (tools/probe/det_gap.py); the default mode's bar for this comparison is 3e-2 / 0.2
            for k, (x, y) in enumerate(zip(_state(a), _state(c))):
                if x.dtype in (torch.float32, torch.float16):
                    assert float((x.float() - y.float()).norm()) <= 1e-6 * float(x.float().norm()) + 1e-12, f"eager vs rtxn_train_step after ONE step: tensor {k}"
    moved = float((a.master - _small_trainer(torch, encoding, mode, neurons, layers).master).abs().max())
    assert moved > 1e-3 and bool(torch.isfinite(a.master).all())
    # the one-call step: the same gradient kernels, but its Adam takes beta^t from the device step counter (v_exp_f32, 1e-6 relative on
    # the learning rate): equal to 1e-6 after one step (above), and what is left of that after six
    for k, (x, y) in enumerate(zip(_state(a), _state(c))):
        if x.dtype in (torch.float32, torch.float16):
            assert float((x.float() - y.float()).norm()) <= 3e-2 * float(x.float().norm()) + 1e-12, f"eager vs rtxn_train_step: tensor {k}"   # six steps at lr 1e-2 amplify the 1e-7 of step one 30x per step on the moments (measured 2e-3 ... 1.4e-2 by build, tools/probe/det_gap.py): the sharp statement is the one-step bar above
    # the shadows are left clean, and the default mode is untouched by a deterministic trainer living in the same process
    assert int(a._det_mlp.abs().max()) == 0 and (a._det_table is None or int(a._det_table.abs().max()) == 0)
    plain = _small_trainer(torch, encoding, mode, neurons, layers)
    assert not plain.deterministic
    o, d, t = batches[0]
    plain.step(o, d, t)
    ref = _small_trainer(torch, encoding, mode, neurons, layers, deterministic=True)
    ref.step(o, d, t)
    torch.cuda.synchronize()
    pa, pr = plain.master.cpu().numpy(), ref.master.cpu().numpy()
    assert np.linalg.norm(pa - pr) <= 2e-2 * np.linalg.norm(pr)         # the same gradients up to float-atomic noise through one Adam step


def test_deterministic_captured_step_and_checkpoint_resume(gpu, tmp_path):
    """The captured step (hipGraphs, traversal one batch ahead) in deterministic mode: two trainers bit-identical after eight
    replays; and a checkpoint written after four steps, loaded into a fresh trainer and stepped four more, ends bit-identical
    to the uninterrupted run (default mode: 5e-4, tests/test_gpu_harness.py)."""
    torch = gpu
    batches = _det_batches(torch, n=8)
    B = batches[0][0].shape[0]
    runs = []
    for _ in range(2):
        tr = _small_trainer(torch, "hash", "nerf", 64, 4, deterministic=True)
        tr.capture_step(B, launch_segments=B * 30, prefetch=True)
        for o, d, t in batches:
            tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
            tr.step_captured()
        tr.flush_captured()
        torch.cuda.synchronize()
        runs.append(_state(tr))
    for k, (x, y) in enumerate(zip(*runs)):
        assert torch.equal(x, y), f"captured vs captured: tensor {k}"
    full = _small_trainer(torch, "hash", "nerf", 64, 4, deterministic=True)
    half = _small_trainer(torch, "hash", "nerf", 64, 4, deterministic=True)
    path = str(tmp_path / "det.ckpt")
    for i, (o, d, t) in enumerate(batches):
        full.step(o, d, t)
        if i < 4:
            half.step(o, d, t)
    half.save_checkpoint(path)
    resumed = _small_trainer(torch, "hash", "nerf", 64, 4, seed=99, deterministic=True)
    resumed.load_checkpoint(path)
    for o, d, t in batches[4:]:
        resumed.step(o, d, t)
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(_state(full), _state(resumed))):
        assert torch.equal(x, y), f"resumed vs uninterrupted: tensor {k}"


def _reference_model_trainer(torch, **kw):
    """The reference's own model (8 x 128, Composite-Frequency(3 x 10, 2 x 12): 112 encoded features) on a small scene"""
    import numpy as np
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import Trainer
    R, B = 16, 900
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()
    return Trainer(R, occ, encoding="freq", n_neurons=128, n_hidden_layers=8, n_dir_freqs=12, batch_rays=B, max_segments=B * 30, lr=1e-3,
                   loss_scale=128.0, mode="compat", seed=3, **kw)


def test_reference_model_fused_staged_and_saved_paths_agree(gpu, monkeypatch):
    """The reference's 8 x 128 model through the Trainer, three eager steps of its own iteration (compat compositor) on the same
    batches: (a) lean with sampler + encoder folded into the forward and the weight gradient (default), (b) lean with the staged
    encoder (RTXN_TRAIN_LEAN_FUSED=0), (c) saved activations (RTXN_TRAIN_LEAN=0), (d) one C call per step (rtxn_train_step, which
    folds the encoder in too).  In deterministic mode (a) and (b) are BIT-IDENTICAL -- the folded encoder produces the staged one's
    operands bit for bit and the gradient sums are order-free -- and (d) matches to the device-side beta^t of its Adam; the saved
    path differs by the rounding points of its weight-gradient sums."""
    torch = gpu
    batches = _det_batches(torch, n=3)
    B = batches[0][0].shape[0]

    def run(env, entry=False):
        for k in ("RTXN_TRAIN_LEAN_FUSED", "RTXN_TRAIN_LEAN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr = _reference_model_trainer(torch, deterministic=True)
        if entry:
            tr.entry_args(B, launch_segments=B * 30)
        for o, d, t in batches:
            if entry:
                tr.graph_rays_o.copy_(o); tr.graph_rays_d.copy_(d); tr.graph_targets.copy_(t)
                tr.step_entry()
            else:
                tr.step(o, d, t)
        torch.cuda.synchronize()
        return tr

    fused = run({})
    staged = run({"RTXN_TRAIN_LEAN_FUSED": "0"})
    saved = run({"RTXN_TRAIN_LEAN": "0"})
    entry = run({}, entry=True)
    assert fused.lean and fused.lean_fused and staged.lean and not staged.lean_fused and not saved.lean and entry.lean_fused
    assert int(fused.total.item()) * 32 > 50_000
    moved = float((fused.master - _reference_model_trainer(torch).master).abs().max())
    assert moved > 1e-3
    for k, (x, y) in enumerate(zip(_state(fused), _state(staged))):
        assert torch.equal(x, y), f"folded vs staged encoder: tensor {k}: {int((x != y).sum())} of {x.numel()} differ"
    rel = lambda x, y: float((x.float() - y.float()).norm()) / float(x.float().norm())
    assert rel(fused.master, entry.master) <= 1e-5 and rel(fused.master, saved.master) <= 1e-4
    assert torch.equal(fused.t_vals[:1000], staged.t_vals[:1000])
