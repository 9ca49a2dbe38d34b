"""Layer 0 of the 16x16x32 inference kernels with the direction k-steps first: the segment kernel computes their product once
per segment (rtxn::dir_bias16) and starts the position k-steps of both of a segment's column tiles from it, the per-sample
kernel runs the same k-steps in the same order.  Fused (sampler folded in) == staged (sampler, then the per-sample forward)
bit for bit for every fwd16 variant and both segment output forms; a wave's two segments land in their own columns; every
tcnn feature of the new layer-0 order reaches the output exactly once."""
import numpy as np
import pytest

from rtx_nerf_amd import scenes

pytestmark = pytest.mark.gpu

VARIANTS = [(128, 12), (64, 12), (128, 4), (64, 4)]   # (width, direction frequencies): the four fwd16 kernels


def _dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _net(oracle, api, torch, W, df, seed, nh=3):
    cfg = oracle.mlp_cfg(n_neurons=W, n_hidden_layers=nh, n_dir_freqs=df)
    params = scenes.xavier_params_fp16(W, nh, oracle.mlp_enc_padded(cfg), seed=seed)
    net = api.Network(n_neurons=W, n_hidden_layers=nh, n_dir_freqs=df)
    net.set_params(_dev(torch, params))
    return cfg, params, net


def _segments(rng, P, cap):
    """P segments, each its own ray (one view direction per segment), in buffers of cap segments (zeros beyond P)."""
    sp = np.zeros((cap, 3), np.float32)
    ep = np.zeros((cap, 3), np.float32)
    vd = np.zeros((cap, 2), np.float32)
    sp[:P] = rng.uniform(-1, 1, (P, 3))
    ep[:P] = rng.uniform(-1, 1, (P, 3))
    vd[:P] = rng.uniform(-3.1, 3.1, (P, 2))
    return sp, ep, vd


def _fused(torch, net, sp, ep, vd, total, max_segments, compact):
    cap = sp.shape[0]
    tot = torch.tensor([total], dtype=torch.int32, device="cuda")
    if compact:
        out = torch.full((cap * 32, 4), -3.0, dtype=torch.float16, device="cuda")
        net.forward_segments_compact(_dev(torch, sp), _dev(torch, ep), _dev(torch, vd), tot, max_segments, out)
    else:
        out = torch.full((cap * 32, 4), -3.0, device="cuda")
        net.forward_segments(_dev(torch, sp), _dev(torch, ep), _dev(torch, vd), tot, max_segments, out, None)
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("W,df", VARIANTS)
def test_fused_equals_staged_all_variants(gpu, oracle, W, df, compact):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(11 + W + df)
    P, cap = 301, 320                                      # odd: a wave's second segment lies past *total_segments
    cfg, params, net = _net(oracle, api, torch, W, df, seed=5)
    sp, ep, vd = _segments(rng, P, cap)
    got = _fused(torch, net, sp, ep, vd, P, cap, compact)
    nh, idx = np.ones(P, np.int32), np.arange(P, dtype=np.int32)
    samples, _ = oracle.sample(sp[:P], ep[:P], vd[:P], nh, idx, 0)
    s_d = torch.zeros((P * 32, 5), device="cuda")
    t_d = torch.zeros((P * 32,), device="cuda")
    api.launchSampler(_dev(torch, sp), _dev(torch, ep), _dev(torch, vd[:P]), t_d, s_d, P, 8, _dev(torch, nh), _dev(torch, idx), 0)
    staged = net.forward_radiance(s_d).cpu().numpy()
    np.testing.assert_array_equal(got[:P * 32], staged)     # fused == staged, bit for bit (compact: the same fp16 values)
    assert np.all(got[P * 32:] == -3.0)                     # nothing beyond *total_segments
    want = oracle.mlp_forward(cfg, params, samples).astype(np.float32)[:, :4]
    np.testing.assert_allclose(got[:P * 32], want, rtol=0, atol=1e-2)
    assert np.abs(got[:P * 32] - want).mean() < 1e-3


@pytest.mark.parametrize("W,df", VARIANTS)
def test_segment_pairing(gpu, oracle, W, df):
    """Strongly different directions for the two segments of every wave; swapping the view of segments 2w and 2w+1 swaps
    exactly their outputs (a wrong DPP pattern would hand one segment the other's direction product).  Odd total, clamped by
    max_segments."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(7 + W + df)
    cap, total, max_segments = 96, 93, 77                  # 77 live segments: the last wave has one
    _, _, net = _net(oracle, api, torch, W, df, seed=8)
    sp, ep, vd = _segments(rng, total, cap)
    vd[0:total:2] = [0.3, -2.9]
    vd[1:total:2] = [2.8, 2.5]
    vd[:total] += rng.uniform(-0.05, 0.05, (total, 2)).astype(np.float32)
    base = _fused(torch, net, sp, ep, vd, total, max_segments, False)
    sw = vd.copy()
    n_pairs = max_segments // 2
    sw[0:2 * n_pairs:2], sw[1:2 * n_pairs:2] = vd[1:2 * n_pairs:2], vd[0:2 * n_pairs:2]
    swapped = _fused(torch, net, sp, ep, sw, total, max_segments, False)
    assert np.all(base[max_segments * 32:] == -3.0) and np.all(swapped[max_segments * 32:] == -3.0)
    b = base[:2 * n_pairs * 32].reshape(n_pairs, 2, 32, 4)
    s = swapped[:2 * n_pairs * 32].reshape(n_pairs, 2, 32, 4)
    # same positions, the other segment's direction: compare against a run where each segment carries the other's view
    # through the per-sample path (the positions stay, so outputs are not a plain swap -- the DIRECTION products are)
    nh, idx = np.ones(max_segments, np.int32), np.arange(max_segments, dtype=np.int32)
    s_d = torch.zeros((max_segments * 32, 5), device="cuda")
    t_d = torch.zeros((max_segments * 32,), device="cuda")
    api.launchSampler(_dev(torch, sp), _dev(torch, ep), _dev(torch, sw[:max_segments]), t_d, s_d, max_segments, 8,
                      _dev(torch, nh), _dev(torch, idx), 0)
    staged = net.forward_radiance(s_d).cpu().numpy()
    np.testing.assert_array_equal(swapped[:max_segments * 32], staged)
    assert not np.array_equal(b, s)                        # the directions matter at all
    # the lone last segment (odd count) still sees its own direction
    np.testing.assert_array_equal(base[(max_segments - 1) * 32:max_segments * 32], swapped[(max_segments - 1) * 32:max_segments * 32])


@pytest.mark.parametrize("W,df", VARIANTS)
def test_swapping_a_pair_swaps_outputs(gpu, oracle, W, df):
    """Segments 2w and 2w+1 identical but for their views: swapping the views swaps the two outputs exactly."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(17 + W + df)
    cap, total = 40, 37
    _, _, net = _net(oracle, api, torch, W, df, seed=12)
    sp, ep, vd = _segments(rng, total, cap)
    sp[1:total:2], ep[1:total:2] = sp[0:total - 1:2], ep[0:total - 1:2]
    vd[0:total:2] = [0.2, -3.0]
    vd[1:total:2] = [2.9, 2.7]
    base = _fused(torch, net, sp, ep, vd, total, cap, False)
    sw = vd.copy()
    sw[0:total - 1:2], sw[1:total - 1:2] = vd[1:total - 1:2], vd[0:total - 1:2]
    swapped = _fused(torch, net, sp, ep, sw, total, cap, False)
    n = (total - 1) // 2
    b = base[:2 * n * 32].reshape(n, 2, 32, 4)
    s = swapped[:2 * n * 32].reshape(n, 2, 32, 4)
    np.testing.assert_array_equal(b[:, 0], s[:, 1])
    np.testing.assert_array_equal(b[:, 1], s[:, 0])
    assert not np.array_equal(b[:, 0], b[:, 1])


@pytest.mark.parametrize("df", [12, 4])
def test_every_feature_reaches_the_output_once(gpu, oracle, df):
    """Selection weights (layer 0 copies four features per pass as +f and -f through the ReLU, the output layer subtracts):
    every tcnn feature, padding included, within 1 fp16 ulp of the oracle's -- a feature placed twice would come out doubled,
    one placed nowhere as zero."""
    torch = gpu
    from rtx_nerf_amd import api
    W, n = 128, 2048
    rng = np.random.default_rng(23)
    x = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0, 3.1416, (n, 1)), rng.uniform(-3.1416, 3.1416, (n, 1))], 1).astype(np.float32)
    cfg = oracle.mlp_cfg(n_neurons=W, n_hidden_layers=1, output_activation=0, n_dir_freqs=df)
    E = oracle.mlp_enc_padded(cfg)
    width = 2 * (3 * 10 + 2 * df)
    want = oracle.encode_freq(cfg, x).astype(np.float32)
    net = api.Network(n_neurons=W, n_hidden_layers=1, output_activation=api.ACT_NONE, n_dir_freqs=df)
    got = np.zeros((n, E), np.float32)
    x_d = _dev(torch, x)
    for f0 in range(0, E, 4):
        p = np.zeros(W * E + 16 * W, np.float16)
        w0, wo = p[:W * E].reshape(W, E), p[W * E:].reshape(16, W)
        for k in range(min(4, E - f0)):
            w0[5 + 9 * k, f0 + k] = 1
            w0[70 + 9 * k, f0 + k] = -1
            wo[k, 5 + 9 * k] = 1
            wo[k, 70 + 9 * k] = -1
        net.set_params(_dev(torch, p))
        got[:, f0:f0 + 4] = net.forward(x_d).cpu().numpy().astype(np.float32)[:, :min(4, E - f0)]
    err = np.abs(got - want)
    assert np.all(got[:, width:] == 1.0)                   # the padding features, each exactly once
    assert err.max() <= 1.0e-3, err.max(axis=0)
