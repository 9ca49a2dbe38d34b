"""GPU parity of the training kernels (through the C ABI) against the oracle.

Bars (oracle "parity unpinned", tcnn restated from its published algorithm):
  encoders        fp16 features: hash grid bit-exact; frequency features differ from the
                  double-precision oracle by at most 1 fp16 ulp (v_sin_f32), < 1 % of them
  MLP forward     fp16 outputs/activations 1e-2 abs, mean < 1e-3 (MFMA summation order)
  MLP backward    dparams / denc: relative L2 error < 2e-2, max error < 3e-2 of the largest entry
                  (fp16 dZ rounding flips + fp32 atomics order)
  hash backward   1e-4 relative (fp32 atomics order vs double)
  L2, Adam        1e-6 relative
"""
import numpy as np
import pytest

from rtx_nerf_amd import scenes

pytestmark = pytest.mark.gpu


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(rng, n):
    return np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0, 3.1416, (n, 1)), rng.uniform(-3.1416, 3.1416, (n, 1))],
                          axis=1).astype(np.float32)


def _ulp_diff(a16, b16):
    a = a16.view(np.int16).astype(np.int32)
    b = b16.view(np.int16).astype(np.int32)
    a = np.where(a < 0, -(a & 0x7fff), a)
    b = np.where(b < 0, -(b & 0x7fff), b)
    return np.abs(a - b)


@pytest.mark.parametrize("n", [1, 255, 1000])
def test_encode_frequency_feature_major(gpu, oracle, n):
    torch = gpu
    from rtx_nerf_amd import api
    x = _inputs(np.random.default_rng(n), n)
    net = api.Network(n_neurons=64, n_hidden_layers=2)
    encT = net.encode_frequency(_dev(torch, x)).cpu().numpy()
    Sp = api.padded_samples(n)
    assert encT.shape == (112, Sp) and Sp % 256 == 0
    want = oracle.encode_freq(oracle.mlp_cfg(n_neurons=64, n_hidden_layers=2), x)
    d = _ulp_diff(encT[:, :n].T.copy(), want)
    # a value that rounds to (almost) zero has a tiny fp16 ulp: compare those absolutely instead
    big = np.abs(want.astype(np.float32)) > 1e-2
    assert d[big].max() <= 1 and (d[big] > 0).mean() < 0.01
    np.testing.assert_allclose(encT[:, :n].T.astype(np.float32), want.astype(np.float32), atol=1e-3)
    assert np.all(encT[:, n:] == 0)            # padding columns are zero
    assert np.all(encT[108:, :n] == 1)         # padding features are one


@pytest.mark.parametrize("levels,feat,log2,base,scale", [(16, 2, 19, 16, 1.5), (4, 2, 10, 4, 1.7), (8, 4, 14, 8, 2.0)])
def test_hashgrid_encode_and_backward(gpu, oracle, levels, feat, log2, base, scale):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(levels)
    n = 3000
    x = _inputs(rng, n)
    hg = api.HashGrid(levels, feat, log2, base, scale, n_dir_freqs=4)
    ocfg = oracle.hg_cfg(levels, feat, log2, base, scale)
    assert hg.n_params() == oracle.hg_n_params(ocfg) and hg.encoded_width() == oracle.hg_enc_width(ocfg, 4)
    table = rng.uniform(-1, 1, hg.n_params()).astype(np.float16)
    encT = hg.encode(_dev(torch, table), _dev(torch, x)).cpu().numpy()
    want = oracle.encode_hg(ocfg, 4, table, x)
    nh = levels * feat
    np.testing.assert_array_equal(encT[:nh, :n].T, want[:, :nh])                       # gathers + trilinear: bit-exact
    np.testing.assert_allclose(encT[nh:, :n].T.astype(np.float32), want[:, nh:].astype(np.float32), atol=1e-3)
    assert np.all(encT[:, n:] == 0)
    # backward: scatter-add of a random denc
    E, Sp = hg.encoded_width(), api.padded_samples(n)
    denc = np.zeros((E, Sp), np.float16)
    denc[:, :n] = rng.standard_normal((E, n)).astype(np.float16)
    dtable = torch.zeros(hg.n_params(), device="cuda")
    hg.backward(_dev(torch, x), _dev(torch, denc), dtable)
    want_g = oracle.hg_backward(ocfg, x, denc[:, :n].T.copy())
    got_g = dtable.cpu().numpy()
    assert np.abs(got_g - want_g).max() < 1e-4 * max(1.0, np.abs(want_g).max())
    assert np.count_nonzero(want_g) > 0
    if feat == 2:
        # mixed form: densely stored levels fp32 as above, hashed levels through packed fp16 atomics into an fp16 table
        lo = hg.hashed_offset()
        assert 0 < lo <= hg.n_params() and lo == sum(min((int(np.ceil(base * scale ** l - 1)) + 1) ** 3 // 8 * 8 + (8 if ((int(np.ceil(base * scale ** l - 1)) + 1) ** 3) % 8 else 0), 2 ** log2)
                                                     for l in range(levels) if (int(np.ceil(base * scale ** l - 1)) + 1) ** 3 <= 2 ** log2) * feat
        dt32 = torch.zeros(hg.n_params(), device="cuda")
        dt16 = torch.zeros(hg.n_params() - lo, dtype=torch.float16, device="cuda")
        hg.backward_mixed(_dev(torch, x), _dev(torch, denc), dt32, dt16)
        got32, got16 = dt32.cpu().numpy(), dt16.cpu().numpy().astype(np.float32)
        assert np.all(got32[lo:] == 0)
        assert np.abs(got32[:lo] - want_g[:lo]).max() < 1e-4 * max(1.0, np.abs(want_g).max())
        if lo < hg.n_params():
            # fp16 accumulation in whatever order the atomics arrive: a running sum of n contributions carries up to ~n/2
            # half-ulps of its largest partial sum (n ~ 25 per entry in the smallest table here); measured maxima 2e-3 ...
            # 3.5e-3 of the largest entry from run to run -- the bound below is that order-dependent worst case, the 2-norm
            # bound after it is the tight one
            assert np.abs(got16 - want_g[lo:]).max() < 1e-2 * max(1.0, np.abs(want_g[lo:]).max())
            assert np.linalg.norm(got16 - want_g[lo:]) < 1e-3 * np.linalg.norm(want_g[lo:])


def _train_case(oracle, api, torch, W, L, E, act, n, seed, use_freq=False):
    rng = np.random.default_rng(seed)
    params = scenes.xavier_params_fp16(W, L, E, seed=seed)
    enc = rng.uniform(-1, 1, (n, E)).astype(np.float16)
    Sp = api.padded_samples(n)
    encT = np.zeros((E, Sp), np.float16)
    encT[:, :n] = enc.T
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E, output_activation=act)
    assert net.n_params() == params.size and net.encoded_width() == E
    net.set_params(_dev(torch, params))
    return net, params, enc, _dev(torch, encT), Sp


@pytest.mark.parametrize("W,L,E,act,n", [(64, 4, 48, 1, 1000), (128, 8, 112, 1, 700), (64, 1, 16, 0, 5), (128, 2, 48, 0, 513),
                                         (64, 5, 112, 1, 256), (128, 3, 112, 1, 5000)])
def test_mlp_train_forward_and_backward(gpu, oracle, W, L, E, act, n):
    torch = gpu
    from rtx_nerf_amd import api
    net, params, enc, encT_d, Sp = _train_case(oracle, api, torch, W, L, E, act, n, seed=W + L + n)
    ws = net.train_workspace(n)
    rad = torch.zeros((n, 4), device="cuda")
    out = net.train_forward(encT_d, n, ws, radiance=rad)
    torch.cuda.synchronize()
    o_acts, o_out = oracle.mlpe_forward(W, L, act, params, enc)
    got = out.cpu().numpy().astype(np.float32)
    np.testing.assert_allclose(got, o_out.astype(np.float32), rtol=0, atol=1e-2 if act else 3e-2)
    assert np.abs(got - o_out.astype(np.float32)).mean() < (1e-3 if act else 3e-3)
    np.testing.assert_array_equal(rad.cpu().numpy(), got[:, :4])
    acts = ws[:L * W * Sp].reshape(L, W, Sp).cpu().numpy()
    for l in range(L):
        a_got = acts[l, :, :n].T.astype(np.float32)
        np.testing.assert_allclose(a_got, o_acts[l].astype(np.float32), rtol=0, atol=2e-2)
        assert np.all(acts[l, :, n:] == 0)
    # ---- backward, from the GPU's own forward state ----
    rng = np.random.default_rng(7)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    dparams = torch.zeros(net.n_params(), device="cuda")
    dencT = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    net.train_backward(encT_d, out, _dev(torch, dout), n, ws, dparams, dencT)
    torch.cuda.synchronize()
    acts_sm = np.ascontiguousarray(np.transpose(acts[:, :, :n], (0, 2, 1)))      # oracle layout [L][S][W]
    want_dp, want_denc = oracle.mlpe_backward(W, L, act, params, enc, acts_sm, out.cpu().numpy(), dout)
    got_dp = dparams.cpu().numpy()
    scale = np.abs(want_dp).max()
    assert scale > 0
    assert np.abs(got_dp - want_dp).max() < 3e-2 * scale
    assert np.linalg.norm(got_dp - want_dp) < 2e-2 * np.linalg.norm(want_dp)
    assert np.all(got_dp[-16 * W:].reshape(16, W)[4:] == 0)
    got_denc = dencT.cpu().numpy()[:, :n].T.astype(np.float32)
    assert np.linalg.norm(got_denc - want_denc) < 2e-2 * np.linalg.norm(want_denc) + 1e-6
    assert np.all(dencT.cpu().numpy()[:, n:] == 0)
    # accumulate semantics: a second call doubles the gradient
    net.train_backward(encT_d, out, _dev(torch, dout), n, ws, dparams, None)
    np.testing.assert_allclose(dparams.cpu().numpy(), 2 * got_dp, rtol=1e-3, atol=1e-6 * scale + 1e-9)


def test_train_forward_agrees_with_inference_kernel(gpu, oracle):
    """Frequency model: encode_frequency + train_forward == the fused inference kernel (same weights)."""
    torch = gpu
    from rtx_nerf_amd import api
    n = 2000
    x = _inputs(np.random.default_rng(3), n)
    net = api.Network(n_neurons=128, n_hidden_layers=8)
    params = scenes.xavier_params_fp16(128, 8, 112, seed=21)
    net.set_params(_dev(torch, params))
    x_d = _dev(torch, x)
    ref = net.forward(x_d).cpu().numpy().astype(np.float32)
    encT = net.encode_frequency(x_d)
    out = net.train_forward(encT, n, net.train_workspace(n)).cpu().numpy().astype(np.float32)
    np.testing.assert_allclose(out, ref, rtol=0, atol=4e-3)
    assert (out == ref).mean() > 0.9


def test_l2_loss_and_adam(gpu, oracle):
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(0)
    n = 12288 + 5
    pred = rng.uniform(0, 1, n).astype(np.float32)
    tgt = rng.uniform(0, 1, n).astype(np.float32)
    values = torch.zeros(n, device="cuda")
    grads = torch.zeros(n, dtype=torch.float16, device="cuda")
    total = torch.full((1,), 99.0, device="cuda")
    api.l2_loss(_dev(torch, pred), _dev(torch, tgt), 128.0, values, grads, total)
    w_tot, w_val, w_g16, _ = oracle.l2_loss(pred, tgt, 128.0)
    np.testing.assert_allclose(values.cpu().numpy(), w_val, rtol=1e-6)
    np.testing.assert_array_equal(grads.cpu().numpy(), w_g16)
    assert abs(float(total.item()) - w_tot) < 1e-6 * w_tot + 1e-9
    # Adam, three steps
    k = 100_003
    master = rng.standard_normal(k).astype(np.float32)
    m = np.zeros(k, np.float32)
    v = np.zeros(k, np.float32)
    md, p16d = _dev(torch, master), torch.zeros(k, dtype=torch.float16, device="cuda")
    mm, vv = torch.zeros(k, device="cuda"), torch.zeros(k, device="cuda")
    for step in (1, 2, 3):
        g = (rng.standard_normal(k) * 10.0 ** rng.integers(-6, 1, k)).astype(np.float32)
        api.adam_step(md, p16d, _dev(torch, g), mm, vv, step, lr=1e-2, loss_scale=4.0)
        p16 = oracle.adam_step(master, g, m, v, step, lr=1e-2, loss_scale=4.0)
    np.testing.assert_allclose(md.cpu().numpy(), master, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(vv.cpu().numpy(), v, rtol=1e-5, atol=1e-30)
    assert (p16d.cpu().numpy() == p16).mean() > 0.9999


@pytest.mark.parametrize("L,E,act,n", [(4, 48, 1, 5000), (4, 48, 1, 256), (1, 16, 0, 5), (2, 32, 1, 777), (3, 64, 0, 2049), (4, 64, 1, 70000)])
def test_recompute_path_matches_oracle_and_three_kernel_path(gpu, oracle, L, E, act, n):
    """The 64-wide recompute path (forward without saved activations + mlp_bwd_fused64_kernel: activations rebuilt in
    registers, weight gradients accumulated on the chip through LDS-transposed operands) against the oracle and against the
    saved-activation kernels on the same inputs, ragged sizes and several persistent-loop depths included."""
    torch = gpu
    from rtx_nerf_amd import api
    W = 64
    net, params, enc, encT_d, Sp = _train_case(oracle, api, torch, W, L, E, act, n, seed=L * 100 + E + n)
    assert net.recompute_supported()
    rad = torch.zeros((n, 4), device="cuda")
    out = net.train_forward_outputs(encT_d, n, radiance=rad)
    ws = net.train_workspace(n)
    out_ref = net.train_forward(encT_d, n, ws)
    torch.cuda.synchronize()
    # the outputs-only forward runs the 16x16x32 all-asm layer stack (hashmlp.hip), the saving forward the 32x32x16 one: the same
    # fp16 products summed in another order inside the matrix core -- fp16-ulp differences on a minority of the outputs
    d = (out.float() - out_ref.float()).abs()
    assert float(d.max()) <= 2e-3 * max(1.0, float(out_ref.float().abs().max())) and float((d > 0).float().mean()) < 0.25
    np.testing.assert_array_equal(rad.cpu().numpy(), out.cpu().numpy().astype(np.float32)[:, :4])
    rng = np.random.default_rng(11)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    dout_d = _dev(torch, dout)
    dp, dp_ref = torch.zeros(net.n_params(), device="cuda"), torch.zeros(net.n_params(), device="cuda")
    de = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    de_ref = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    net.train_backward_recompute(encT_d, out, dout_d, n, dp, de)
    net.train_backward(encT_d, out, dout_d, n, ws, dp_ref, de_ref)
    torch.cuda.synchronize()
    o_acts, _ = oracle.mlpe_forward(W, L, act, params, enc)
    want_dp, want_denc = oracle.mlpe_backward(W, L, act, params, enc, o_acts, out.cpu().numpy(), dout)
    got_dp, ref_dp = dp.cpu().numpy(), dp_ref.cpu().numpy()
    scale = np.abs(want_dp).max()
    assert scale > 0 and np.isfinite(got_dp).all()
    assert np.abs(got_dp - want_dp).max() < 3e-2 * scale and np.linalg.norm(got_dp - want_dp) < 2e-2 * np.linalg.norm(want_dp)
    # against the three-kernel path: the same fp16 dZ values, only the fp32 summation order differs
    assert np.linalg.norm(got_dp - ref_dp) < 2e-3 * np.linalg.norm(ref_dp)
    assert np.all(got_dp[-16 * W:].reshape(16, W)[4:] == 0)
    assert torch.equal(de, de_ref)                                         # d(encoding): the identical dgrad chain
    got_denc = de.cpu().numpy()[:, :n].T.astype(np.float32)
    assert np.linalg.norm(got_denc - want_denc) < 2e-2 * np.linalg.norm(want_denc) + 1e-6
    assert np.all(de.cpu().numpy()[:, n:] == 0)
    net.train_backward_recompute(encT_d, out, dout_d, n, dp, None)          # accumulate semantics
    np.testing.assert_allclose(dp.cpu().numpy(), 2 * got_dp, rtol=1e-3, atol=1e-6 * scale + 1e-9)


def test_recompute_path_is_refused_where_it_does_not_fit(gpu):
    torch = gpu
    from rtx_nerf_amd import _lib, api
    for kw in (dict(n_neurons=128, n_hidden_layers=2, n_encoded_features=48), dict(n_neurons=64, n_hidden_layers=5, n_encoded_features=48),
               dict(n_neurons=64, n_hidden_layers=2, n_encoded_features=112)):
        net = api.Network(**kw)
        net.set_params(torch.zeros(net.n_params(), dtype=torch.float16, device="cuda"))
        assert not net.recompute_supported()
        E = kw["n_encoded_features"]
        with pytest.raises(_lib.RtxnError, match="use rtxn_mlp_train_forward"):
            net.train_backward_recompute(torch.zeros((E, 256), dtype=torch.float16, device="cuda"),
                                         torch.zeros((256, 16), dtype=torch.float16, device="cuda"),
                                         torch.zeros((256, 4), dtype=torch.float16, device="cuda"), 256,
                                         torch.zeros(net.n_params(), device="cuda"))


@pytest.mark.parametrize("stype", [0, 3])
def test_sampler_folded_into_encoders_and_scatter(gpu, oracle, stype):
    """rtxn_*_segments (launchSampler folded into its consumers) == rtxn_sample followed by the sample-input entry points:
    encodings and t_vals bit for bit, the scatter up to atomics order."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(stype)
    B, P = 300, 0
    nh = rng.integers(0, 9, B).astype(np.int32)
    P = int(nh.sum())
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
    sp = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    ep = (sp + rng.uniform(-0.05, 0.05, (P, 3))).astype(np.float32)
    vd = np.stack([rng.uniform(0, 3.1, B), rng.uniform(-3.1, 3.1, B)], 1).astype(np.float32)
    sv = vd[np.repeat(np.arange(B), nh)]
    S = P * 32
    sp_d, ep_d, vd_d, sv_d = (_dev(torch, a) for a in (sp, ep, vd, sv))
    samples = torch.zeros((S, 5), device="cuda")
    t_ref = torch.zeros(S, device="cuda")
    api.launchSampler(sp_d, ep_d, vd_d, t_ref, samples, B, 8, _dev(torch, nh), _dev(torch, idx), stype)
    scale = 37.5
    if stype == 3:
        t_ref.mul_(scale)
    Sp = api.padded_samples(S)
    # hash grid
    hg = api.HashGrid(8, 2, 14, 8, 1.6, n_dir_freqs=4)
    table = _dev(torch, rng.uniform(-1, 1, hg.n_params()).astype(np.float16))
    E = hg.encoded_width()
    enc_ref = hg.encode(table, samples)
    enc = torch.full((E, Sp), 3.0, dtype=torch.float16, device="cuda")
    t_got = torch.full((S,), -1.0, device="cuda")
    hg.encode_segments(table, sp_d, ep_d, sv_d, P, stype, enc, t_got, scale)
    assert torch.equal(enc, enc_ref) and torch.equal(t_got, t_ref)
    denc = _dev(torch, np.pad((rng.standard_normal((E, S)) * 0.1).astype(np.float16), ((0, 0), (0, Sp - S))))
    for half in (False, True):
        lo = hg.hashed_offset()
        a32, b32 = torch.zeros(hg.n_params(), device="cuda"), torch.zeros(hg.n_params(), device="cuda")
        a16 = torch.zeros(hg.n_params() - lo, dtype=torch.float16, device="cuda") if half else None
        b16 = torch.zeros(hg.n_params() - lo, dtype=torch.float16, device="cuda") if half else None
        hg.backward_segments(sp_d, ep_d, P, stype, denc, a32, a16)
        if half:
            hg.backward_mixed(samples, denc, b32, b16)
            assert float((a16.float() - b16.float()).abs().max()) <= 1e-2 * float(b16.float().abs().max())   # two fp16 atomic orders
        else:
            hg.backward(samples, denc, b32)
        assert float((a32 - b32).abs().max()) <= 1e-5 * float(b32.abs().max()) and float(b32.abs().max()) > 0
    # frequency encoding
    net = api.Network(n_neurons=64, n_hidden_layers=2)
    f_ref = net.encode_frequency(samples)
    f_got = torch.full((112, Sp), 3.0, dtype=torch.float16, device="cuda")
    t_got.fill_(-1.0)
    net.encode_frequency_segments(sp_d, ep_d, sv_d, P, stype, f_got, t_got, scale)
    assert torch.equal(f_got, f_ref) and torch.equal(t_got, t_ref)


def test_fused_compositor_l2_backward_matches_the_three_calls(gpu, oracle):
    """rtxn_volrender_l2_train == launch_volrender_cuda(NERF) -> L2 loss->evaluate -> launch_volrender_backward_cuda(NERF),
    and both == the oracle chain; ragged rays incl. rays without samples."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(5)
    B, K, ls = 777, 32, 128.0
    nh = rng.integers(0, 12, B).astype(np.int32)
    nh[::7] = 0
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
    P = int(nh.sum())
    rad = np.concatenate([rng.uniform(0, 1, (P * K, 3)), rng.uniform(0, 1, (P * K, 1))], 1).astype(np.float32)
    step = rng.uniform(0.0, 0.2, P * K).astype(np.float32)
    tgt = rng.uniform(0, 1, (B, 3)).astype(np.float32)
    d = {k: _dev(torch, v) for k, v in dict(rad=rad, step=step, nh=nh, idx=idx, tgt=tgt).items()}
    pix, lg, loss = torch.zeros((B, 3), device="cuda"), torch.zeros((B, 3), dtype=torch.float16, device="cuda"), torch.full((1,), 9.0, device="cuda")
    out = torch.zeros((P * K, 4), dtype=torch.float16, device="cuda")
    api.volrender_l2_train(d["rad"], d["step"], d["nh"], d["idx"], B, K, d["tgt"], ls, pix, lg, loss, out)
    pix2, lg2, loss2 = torch.zeros_like(pix), torch.zeros_like(lg), torch.zeros(1, device="cuda")
    out2 = torch.zeros_like(out)
    api.launch_volrender_cuda(None, d["rad"], d["nh"], d["idx"], d["step"], B, K, pix2, mode=api.VR_NERF)
    api.l2_loss(pix2, d["tgt"], ls, None, lg2, loss2)
    api.launch_volrender_backward_cuda(None, lg2, d["rad"], d["step"], d["nh"], d["idx"], B, K, out2, mode=api.VR_NERF)
    torch.cuda.synchronize()
    np.testing.assert_allclose(pix.cpu().numpy(), pix2.cpu().numpy(), rtol=0, atol=2e-6)
    assert abs(float(loss.item()) - float(loss2.item())) < 1e-5 * float(loss2.item())
    assert (lg.cpu().numpy().view(np.uint16) == lg2.cpu().numpy().view(np.uint16)).mean() > 0.999    # same fp16 loss gradients
    a, b = out.cpu().numpy().astype(np.float32), out2.cpu().numpy().astype(np.float32)
    np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-6)
    # oracle chain
    want_pix = oracle.volrender_fwd_nerf(rad, nh, idx, step, K=K)
    np.testing.assert_allclose(pix.cpu().numpy(), want_pix, rtol=0, atol=2e-5)
    o_loss, _, g16, _ = oracle.l2_loss(want_pix, tgt, ls)
    assert abs(float(loss.item()) - o_loss) < 1e-4 * o_loss
    want = oracle.volrender_bwd_nerf(lg.cpu().numpy(), rad, step, nh, idx, K=K)[:P * K]
    np.testing.assert_allclose(a, want, rtol=1.5e-3, atol=2e-5)


def test_live_segment_backward_equals_the_full_backward(gpu):
    """rtxn_live_segments + the two _live backward entry points against the unrestricted calls on a batch whose radiance
    gradient is zero on most segments (as in NeRF training): the list is exactly the segments with a non-zero gradient, in
    ascending order; weight and table gradients agree to the order of the atomics; d(encoding) of the listed segments is
    identical, the other columns are left alone."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(11)
    P, K = 700, 32
    S = P * K
    hg = api.HashGrid(8, 2, 14, 8, 1.6, n_dir_freqs=4)
    E = hg.encoded_width()
    net = api.Network(n_neurons=64, n_hidden_layers=3, n_encoded_features=E)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(64, 3, E, seed=4)))
    sp = rng.uniform(-0.9, 0.9, (P, 3)).astype(np.float32)
    ep = (sp + rng.uniform(-0.02, 0.02, (P, 3))).astype(np.float32)
    sv = rng.uniform(0, 3, (P, 2)).astype(np.float32)
    sp_d, ep_d, sv_d = _dev(torch, sp), _dev(torch, ep), _dev(torch, sv)
    table = _dev(torch, rng.uniform(-1, 1, hg.n_params()).astype(np.float16))
    Sp = api.padded_samples(S)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    t_vals = torch.zeros(S, device="cuda")
    hg.encode_segments(table, sp_d, ep_d, sv_d, P, api.SAMPLING_REGULAR, encT, t_vals, 1.0)
    out = torch.zeros((S, 16), dtype=torch.float16, device="cuda")
    rad = torch.zeros((S, 4), device="cuda")
    net.train_forward_outputs(encT, S, out, rad)
    live = np.zeros(P, bool)
    live[rng.choice(P, 90, replace=False)] = True
    live[[0, P - 1]] = True
    dout = np.zeros((P, K, 4), np.float16)
    dout[live] = (rng.standard_normal((int(live.sum()), K, 4)) * 0.05).astype(np.float16)
    dout[live, 1:, :] *= (rng.uniform(size=(int(live.sum()), K - 1, 1)) < 0.5)     # some zero samples inside live segments
    dout[5, :, :] = 0
    dout[5, 7, 2] = np.float16(-0.0)                                             # -0.0 is zero: segment 5 stays dead
    live[5] = False
    dout_d = _dev(torch, dout.reshape(S, 4))
    cap = P + 37
    ws = api.live_segments_workspace(cap)
    api.live_segments(dout_d, P, cap, ws)
    n = int(ws[0].item())
    np.testing.assert_array_equal(ws[4:4 + n].cpu().numpy(), np.nonzero(live)[0])
    # full backward
    dp_full = torch.zeros(net.n_params(), device="cuda")
    de_full = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    net.train_backward_recompute(encT, out, dout_d, S, dp_full, de_full)
    lo = hg.hashed_offset()
    dt_full, dh_full = torch.zeros(hg.n_params(), device="cuda"), torch.zeros(hg.n_params() - lo, dtype=torch.float16, device="cuda")
    hg.backward_segments(sp_d, ep_d, P, api.SAMPLING_REGULAR, de_full, dt_full, dh_full)
    # live backward
    dp_live = torch.zeros(net.n_params(), device="cuda")
    de_live = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    net.train_backward_recompute_live(encT, out, dout_d, S, ws, dp_live, de_live)
    dt_live, dh_live = torch.zeros(hg.n_params(), device="cuda"), torch.zeros(hg.n_params() - lo, dtype=torch.float16, device="cuda")
    hg.backward_segments(sp_d, ep_d, P, api.SAMPLING_REGULAR, de_live, dt_live, dh_live, live_ws=ws)
    assert float((dp_full - dp_live).norm()) <= 1e-5 * float(dp_full.norm()) and float(dp_full.norm()) > 0
    cols = np.repeat(live, K)
    a, b = de_full.cpu().numpy()[:, :S], de_live.cpu().numpy()[:, :S]
    np.testing.assert_array_equal(a[:, cols], b[:, cols])
    assert np.all(b[:, ~cols] == 7.0) and np.all(a[:, ~cols] == 0.0)
    assert float((dt_full - dt_live).abs().max()) <= 1e-5 * float(dt_full.abs().max()) and float(dt_full.abs().max()) > 0
    assert float((dh_full.float() - dh_live.float()).abs().max()) <= 1e-2 * float(dh_full.float().abs().max())   # two fp16 atomic orders
    assert float((dh_full.float() - dh_live.float()).norm()) <= 2e-3 * float(dh_full.float().norm())
    # nothing live: count 0, gradients untouched
    api.live_segments(torch.zeros_like(dout_d), P, cap, ws)
    assert int(ws[0].item()) == 0
    dp0 = torch.zeros(net.n_params(), device="cuda")
    net.train_backward_recompute_live(encT, out, torch.zeros_like(dout_d), S, ws, dp0, de_live)
    assert float(dp0.abs().max()) == 0.0


@pytest.mark.parametrize("W,L", [(128, 3), (64, 2)])
def test_live_segment_backward_of_the_saved_activation_path(gpu, W, L):
    """rtxn_mlp_train_backward_live (dgrad chain over the live segments, dZ written compactly, weight-gradient kernels
    contracting over the list) against rtxn_mlp_train_backward on the same saved activations: same weight gradients to fp32
    atomic order, identical d(encoding) on the listed segments.  Segment counts chosen so that the list ends inside a
    256-sample tile and inside a weight-gradient chunk."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(W + L)
    P, K, E = 330, 32, 48
    S = P * K
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(W, L, E, seed=9)))
    Sp = api.padded_samples(S)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    encT[:, :S] = _dev(torch, rng.uniform(-1, 1, (E, S)).astype(np.float16))
    ws = net.train_workspace(S)
    out = torch.zeros((S, 16), dtype=torch.float16, device="cuda")
    net.train_forward(encT, S, ws, out, None)
    live = np.zeros(P, bool)
    live[rng.choice(P, 75, replace=False)] = True
    live[[0, P - 1]] = True
    dout = np.zeros((P, K, 4), np.float16)
    dout[live] = (rng.standard_normal((int(live.sum()), K, 4)) * 0.05).astype(np.float16)
    dout_d = _dev(torch, dout.reshape(S, 4))
    lws = api.live_segments_workspace(P)
    api.live_segments(dout_d, P, P, lws)
    assert int(lws[0].item()) == int(live.sum())
    dp_full = torch.zeros(net.n_params(), device="cuda")
    de_full = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    ws_full = ws.clone()
    net.train_backward(encT, out, dout_d, S, ws_full, dp_full, de_full)
    dp_live = torch.zeros(net.n_params(), device="cuda")
    de_live = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    ws_live = ws.clone()
    net.train_backward_live(encT, out, dout_d, S, ws_live, lws, dp_live, de_live)
    assert float(dp_full.norm()) > 0 and float((dp_full - dp_live).norm()) <= 1e-5 * float(dp_full.norm())
    cols = np.repeat(live, K)
    a, b = de_full.cpu().numpy()[:, :S], de_live.cpu().numpy()[:, :S]
    np.testing.assert_array_equal(a[:, cols], b[:, cols])
    assert np.all(b[:, ~cols] == 7.0)
    # Two-pass forward (round 3): outputs for everything (no workspace), activations for the LIVE segments only, saved into
    # the workspace where the one-pass forward puts them; the live backward on that workspace gives the same results, and
    # nothing outside the listed segments' columns is written (the fill value survives there).
    out2 = net.train_forward_outputs(encT, S)
    d = (out2.float() - out.float()).abs()
    assert float(d.max()) <= 2e-3            # W = 64: 16x16x32 layer stack vs the saving kernel's 32x32x16 (fp16-ulp); W = 128: same kernel
    if W == 128:
        assert torch.equal(out2, out)
    ws2 = torch.full_like(ws, 3.0)
    net.train_forward_live(encT, S, ws2, lws)
    acts_full = ws[:L * W * Sp].view(L, W, Sp)[:, :, :S].cpu().numpy()
    acts_live = ws2[:L * W * Sp].view(L, W, Sp)[:, :, :S].cpu().numpy()
    np.testing.assert_array_equal(acts_live[:, :, cols], acts_full[:, :, cols])
    assert np.all(acts_live[:, :, ~cols] == 3.0)
    dp2 = torch.zeros(net.n_params(), device="cuda")
    de2 = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    net.train_backward_live(encT, out, dout_d, S, ws2, lws, dp2, de2)
    assert float((dp2 - dp_live).norm()) <= 1e-5 * float(dp_live.norm())
    np.testing.assert_array_equal(de2.cpu().numpy()[:, :S][:, cols], b[:, cols])


@pytest.mark.parametrize("W,L,E", [(128, 1, 48), (128, 2, 48), (128, 3, 48), (128, 4, 112), (128, 8, 48), (64, 2, 48), (64, 3, 112)])
def test_outputs_only_forward_against_saving_forward_and_torch_per_column_tile(gpu, W, L, E):
    """Round 3: hipcc hoisted the caller's first conversion above the asm statement that spends the MFMA-result wait states,
    and the outputs-only 128-wide forward read two accumulator elements of column tile 1 one k-step short, in every layer
    (errors ~2e-2 at the outputs: inside the tolerance of the oracle comparison above, which is why this test compares tightly
    and per 32-sample column tile).  Same kernel family -> bit-equal at W = 128; the 64-wide outputs-only forward runs the
    16x16x32 stack (fp16-ulp apart)."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(W + L + E)
    S = 330 * 32
    params = scenes.xavier_params_fp16(W, L, E, seed=9)
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E)
    net.set_params(_dev(torch, params))
    Sp = api.padded_samples(S)
    enc = rng.uniform(-1, 1, (E, S)).astype(np.float16)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    encT[:, :S] = _dev(torch, enc)
    saved = net.train_forward(encT, S, net.train_workspace(S)).float()
    outs = net.train_forward_outputs(encT, S).float()
    p = _dev(torch, params).float()
    x = _dev(torch, enc).float().T
    off = 0
    for width_in in [E] + [W] * (L - 1):
        x = torch.relu(x @ p[off:off + W * width_in].view(W, width_in).T).half().float()
        off += W * width_in
    want = torch.sigmoid(x @ p[off:off + 16 * W].view(16, W).T)
    ct = (torch.arange(S, device="cuda") % 64) // 32
    for got in (saved, outs):
        for c in (0, 1):
            assert float((got - want)[ct == c].abs().max()) < 1.5e-3        # sigmoid outputs: 3 fp16 ulps at 0.5..1
    if W == 128:
        assert torch.equal(saved, outs)


@pytest.mark.parametrize("half_grads", [False, True])
def test_adam_sparse_matches_oracle(gpu, oracle, half_grads):
    """rtxn_adam_step_sparse (the hash table's optimizer) against oracle.adam_step_sparse over five steps of gradients that are
    zero on a different 90 % of the entries each time: identical update counts, weights and moments to fp32 rounding of the
    in-kernel bias correction (one exp2 per power; the oracle's is powf), untouched entries bit-identical to where they started; ZERO clears what it consumed."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(11)
    n = 10_003
    master = rng.standard_normal(n).astype(np.float32) * 1e-2
    m, v, st = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    md, mm, vv = _dev(torch, master.copy()), _dev(torch, m.copy()), _dev(torch, v.copy())
    sd = torch.zeros(n, dtype=torch.int32, device="cuda")
    p16d = torch.zeros(n, dtype=torch.float16, device="cuda")
    start = master.copy()
    never = np.ones(n, bool)
    for step in range(5):
        g = (rng.standard_normal(n) * 0.3).astype(np.float16 if half_grads else np.float32)
        g[rng.uniform(size=n) < 0.9] = 0
        if step == 2:
            g[:64] = 0                                    # whole 4-parameter groups and waves without a gradient
        never &= g == 0
        gd = _dev(torch, g.copy())
        api.adam_step_sparse(md, p16d, gd, mm, vv, sd, lr=1e-2, eps=1e-15, loss_scale=4.0, zero_grads=(step % 2 == 0))
        oracle.adam_step_sparse(master, g.astype(np.float32), m, v, st, lr=1e-2, eps=1e-15, loss_scale=4.0)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(sd.cpu().numpy().view(np.uint32), st)
        np.testing.assert_allclose(md.cpu().numpy(), master, rtol=0, atol=3e-7)
        np.testing.assert_allclose(mm.cpu().numpy(), m, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(vv.cpu().numpy(), v, rtol=1e-6, atol=1e-12)
        left = gd.cpu().numpy()
        assert not left.any() if step % 2 == 0 else np.array_equal(left, g)
        touched = st > 0
        np.testing.assert_array_equal(p16d.cpu().numpy()[touched], md.cpu().numpy()[touched].astype(np.float16))
    assert never.any() and np.array_equal(md.cpu().numpy()[never], start[never]) and not st[never].any()


def test_half2_sparse_gradient_primitives(gpu):
    """rtxn_half2_count_nonzero / _pack_nonzero / _add_pairs (the device side of rtx_nerf_amd/dp.py): counts per block, a list
    that holds exactly the non-zero entries of the masked blocks (any order, -0 is zero), the masked blocks cleared, capacity
    respected with the full need reported, and pack -> add restoring the gradient bit for bit."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(3)
    block, nb = 1 << 12, 5
    n = block * nb - 100                                   # ragged last block
    v = np.zeros((n, 2), np.float16)
    dens = [0.5, 0.01, 0.0, 0.2, 0.03]
    for b in range(nb):
        lo, hi = b * block, min(n, (b + 1) * block)
        at = lo + np.nonzero(rng.uniform(size=hi - lo) < dens[b])[0]
        v[at] = rng.standard_normal((at.size, 2)).astype(np.float16)
        v[at[::7], 1] = 0                                  # entries with one zero half still count
    v[block + 5] = (np.float16(-0.0), np.float16(0.0))
    nz = (v.view(np.uint16) & 0x7fff).any(axis=1)
    vals = _dev(torch, v.reshape(-1).copy())
    counts_d, ws = api.half2_count_nonzero(vals, block)
    counts = counts_d.cpu().numpy()
    want_counts = [int(nz[b * block:(b + 1) * block].sum()) for b in range(nb)]
    assert counts.tolist() == want_counts
    mask = 0b11010                                         # blocks 1, 3, 4
    need = want_counts[1] + want_counts[3] + want_counts[4]
    pairs = torch.zeros((need + 10, 2), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    api.half2_pack_nonzero(vals, block, ws, mask, pairs, cnt, clear=True)
    assert int(cnt.item()) == need
    got = pairs[:need].cpu().numpy()
    assert (np.diff(got[:, 0]) > 0).all()                  # ascending entry index: the same list on every run
    sel = np.zeros(n, bool)
    for b in (1, 3, 4):
        sel[b * block:(b + 1) * block] = True
    want_idx = np.nonzero(nz & sel)[0]
    order = np.argsort(got[:, 0])
    np.testing.assert_array_equal(got[order, 0], want_idx)
    np.testing.assert_array_equal(got[order, 1].view(np.uint32), v.view(np.uint32).reshape(-1)[want_idx])
    after = vals.cpu().numpy().reshape(n, 2)
    assert not after[sel].view(np.uint16).any()            # masked blocks cleared (the -0 too)
    np.testing.assert_array_equal(after[~sel].view(np.uint16), v[~sel].view(np.uint16))
    api.half2_add_pairs(vals, pairs, need)                 # 0 + x = x: the gradient is back
    back = vals.cpu().numpy().reshape(n, 2)
    np.testing.assert_array_equal(back[nz].view(np.uint16), v[nz].view(np.uint16))
    assert not back[~nz].view(np.uint16).any()
    api.half2_add_pairs(vals, pairs, need)                 # fp16 adds: x + x
    twice = vals.cpu().numpy().reshape(n, 2)
    np.testing.assert_array_equal(twice[sel], (v[sel].astype(np.float32) * 2).astype(np.float16))
    # capacity smaller than the need: the list is cut off, the need still reported, nothing written past the capacity
    vals2 = _dev(torch, v.reshape(-1).copy())
    small = torch.full((8, 2), -1, dtype=torch.int32, device="cuda")
    api.half2_pack_nonzero(vals2, block, ws, mask, small[:4], cnt, clear=False)      # ws: counted on the same values
    assert int(cnt.item()) == need and (small[4:] == -1).all() and (small[:4, 0] >= 0).all()
    np.testing.assert_array_equal(vals2.cpu().numpy().view(np.uint16), v.reshape(-1).view(np.uint16))     # clear=False
    # a foreign list with an index past the end is ignored
    bad = torch.tensor([[n + 3, 0x3c003c00], [0, 0]], dtype=torch.int32, device="cuda")
    api.half2_add_pairs(vals2, bad, 1)
    np.testing.assert_array_equal(vals2.cpu().numpy().view(np.uint16), v.reshape(-1).view(np.uint16))


def test_hashgrid_out_of_domain_positions_stay_inside_the_table(gpu, oracle):
    """hg_index_nodiv replaced `% size` by one conditional subtract on the densely stored levels, which only covers
    positions inside [-1, 1]^3.  Out-of-domain and non-finite positions handed to the public encode / backward entry points
    must wrap like hg_index (the oracle's and tcnn's `% size`) and never leave the level: finite out-of-range inputs equal the
    oracle bit for bit; Inf / NaN / huge inputs only have to stay in bounds (no fault on the gathers, guard entries around the
    gradient tables untouched)."""
    torch = gpu
    from rtx_nerf_amd import api
    O = oracle
    hg = api.HashGrid(6, 2, 12, 4, 1.6, n_dir_freqs=4)
    cfg = O.hg_cfg(6, 2, 12, 4, 1.6)
    n_par = hg.n_params()
    assert 0 < hg.hashed_offset() < n_par                   # both kinds of level are exercised
    rng = np.random.default_rng(5)
    table = (rng.uniform(-1, 1, n_par)).astype(np.float16)
    x = rng.uniform(-1, 1, (512, 5)).astype(np.float32)
    x[:128, :3] = rng.uniform(-9, 9, (128, 3))              # finite, far outside the domain, both signs
    x[128:160, 0] = 1.0 + 2.0 ** -20                        # just past the upper face
    got = hg.encode(_dev(torch, table), _dev(torch, x)).cpu().numpy()[:, :512].T
    want = O.encode_hg(cfg, 4, table, x)
    np.testing.assert_array_equal(np.ascontiguousarray(got[:, :12]).view(np.uint16), np.ascontiguousarray(want[:, :12]).view(np.uint16))
    # non-finite / huge: memory safety only.  The table sits between two guard blocks in one allocation.
    bad = x.copy()
    bad[0:8, 0] = np.inf; bad[8:16, 1] = -np.inf; bad[16:24, 2] = np.nan; bad[24:32, :3] = 3.0e38; bad[32:40, :3] = -3.0e38
    G = 4096
    buf = torch.zeros(n_par + 2 * G, dtype=torch.float16, device="cuda")
    buf[G:G + n_par] = _dev(torch, table)
    enc = hg.encode(buf[G:G + n_par], _dev(torch, bad))     # NaN features for the non-finite rows (fr = p - floor(p)): values are not the point
    assert torch.isfinite(enc[:, 40:512].float()).all()
    dtab = torch.zeros(n_par + 2 * G, dtype=torch.float32, device="cuda")
    dtab_h = torch.zeros(n_par - hg.hashed_offset() + 2 * G, dtype=torch.float16, device="cuda")
    denc = torch.ones_like(enc)
    hg.backward(_dev(torch, bad), denc, dtab[G:G + n_par])
    hg.backward_mixed(_dev(torch, bad), denc, dtab[G:G + n_par], dtab_h[G:G + n_par - hg.hashed_offset()])
    torch.cuda.synchronize()
    for t, n in ((dtab, n_par), (dtab_h, n_par - hg.hashed_offset())):
        assert float(t[:G].abs().sum()) == 0.0 and float(t[G + n:].abs().sum()) == 0.0


def test_inference_refuses_stale_weights_after_a_training_only_update(gpu):
    """rtxn_mlp_set_params_training re-packs the training layouts only.  The fused inference kernels must then
    refuse to run (error status, not a fault on a NULL packing and not a silent render with the old weights) until
    rtxn_mlp_set_params is called again."""
    torch = gpu
    from rtx_nerf_amd import api, _lib
    net = api.Network(n_neurons=64, n_hidden_layers=2)
    p = net.initialize_params(3).half().cuda()
    x = torch.rand(256, 5, device="cuda") * 2 - 1
    net.set_params_training(p)                       # never set for inference at all
    with pytest.raises(_lib.RtxnError, match="rtxn_mlp_set_params"):
        net.forward(x)
    net.set_params(p)
    y0 = net.forward(x).clone()
    net.set_params_training((p * 0.5).contiguous())  # a training step's update
    with pytest.raises(_lib.RtxnError, match="stale"):
        net.forward(x)
    net.set_params((p * 0.5).contiguous())
    y1 = net.forward(x)
    assert not torch.equal(y0, y1)


@pytest.mark.parametrize("recompute", [True, False])
def test_live_segments_with_a_saturated_output_leave_no_stale_gradient(gpu, recompute):
    """Round 3: a LISTED segment (non-zero dL/d(radiance)) whose network outputs are saturated -- y == 1.0 or 0.0 in fp16, so
    dZ_out = dout * y (1 - y) is exactly zero in every sample -- made the backward kernels skip its tile without writing its
    d(encoding) columns, and the hash scatter, walking the same list, then added whatever the buffer held (NaNs from
    uninitialised memory poisoned a training run 14 steps in).  A whole tile of such segments: their columns must read zero
    afterwards, and the scatter must add nothing for them."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(3)
    P, K = 24, 32
    S = P * K
    hg = api.HashGrid(4, 2, 12, 8, 1.6, n_dir_freqs=4)
    E = hg.encoded_width()
    net = api.Network(n_neurons=64, n_hidden_layers=2, n_encoded_features=E)
    assert net.recompute_supported()
    net.set_params(_dev(torch, scenes.xavier_params_fp16(64, 2, E, seed=4)))
    sp = rng.uniform(-0.9, 0.9, (P, 3)).astype(np.float32)
    ep = (sp + rng.uniform(-0.02, 0.02, (P, 3))).astype(np.float32)
    sv = rng.uniform(0, 3, (P, 2)).astype(np.float32)
    sp_d, ep_d, sv_d = _dev(torch, sp), _dev(torch, ep), _dev(torch, sv)
    table = _dev(torch, rng.uniform(-1, 1, hg.n_params()).astype(np.float16))
    Sp = api.padded_samples(S)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    hg.encode_segments(table, sp_d, ep_d, sv_d, P, api.SAMPLING_REGULAR, encT, torch.zeros(S, device="cuda"), 1.0)
    ws_act = None if recompute else net.train_workspace(S)
    out = net.train_forward_outputs(encT, S) if recompute else net.train_forward(encT, S, ws_act)
    # segments 8..15 (one whole 8-segment tile of the live walk when segments 0..7 are live too): saturated outputs
    sat = np.zeros(P, bool)
    sat[8:16] = True
    out_np = out.cpu().numpy().reshape(P, K, 16)
    out_np[sat, :, :4] = np.float16(1.0)
    out_np[sat, ::2, 1] = np.float16(0.0)
    out = _dev(torch, out_np.reshape(S, 16))
    dout = (rng.standard_normal((P, K, 4)) * 0.05).astype(np.float16)
    dout[16:] = 0                                             # segments 16.. carry no gradient: not listed
    dout_d = _dev(torch, dout.reshape(S, 4))
    ws = api.live_segments_workspace(P + 5)
    api.live_segments(dout_d, P, P + 5, ws)
    assert int(ws[0].item()) == 16
    dp = torch.zeros(net.n_params(), device="cuda")
    de = torch.full((E, Sp), float("nan"), dtype=torch.float16, device="cuda")      # what uninitialised memory can hold
    if recompute:
        net.train_backward_recompute_live(encT, out, dout_d, S, ws, dp, de)
    else:
        net.train_backward_live(encT, out, dout_d, S, ws_act, ws, dp, de)
    lo = hg.hashed_offset()
    dt, dh = torch.zeros(hg.n_params(), device="cuda"), torch.zeros(hg.n_params() - lo, dtype=torch.float16, device="cuda")
    hg.backward_segments(sp_d, ep_d, P, api.SAMPLING_REGULAR, de, dt, dh, live_ws=ws)
    torch.cuda.synchronize()
    d = de.cpu().numpy()[:, :S].reshape(E, P, K)
    assert np.all(d[:, sat] == 0.0)                           # listed, saturated: zeros, not the NaN fill
    assert np.isfinite(d[:, :8]).all() and np.abs(d[:, :8].astype(np.float32)).max() > 0
    assert np.isnan(d[:, 16:].astype(np.float32)).all()       # not listed: never touched (and never read)
    assert torch.isfinite(dp).all() and torch.isfinite(dt).all() and torch.isfinite(dh.float()).all()
    assert float(dt.abs().max()) > 0


@pytest.mark.parametrize("S", [2_000_000, 3_800_000])
def test_weight_gradient_is_additive_over_the_batch_at_full_size(gpu, S):
    """The reference iteration's batch sizes (millions of samples: the weight-gradient kernel then takes 4096 / 8192 samples per
    block and walks 16 / 32 tiles by its live-tile mask) are out of the oracle's reach, so the check is the size-independent
    property: dW of the whole batch == the sum of dW over seven unequal slices of it, each run as its own small batch (the
    2048-samples-per-block path that the oracle tests and tools/fuzz_train.py cover).  A band of the batch has a zero loss
    gradient (dead tiles in the middle of blocks).  Tolerance: fp32 summation order only (atomics; fp16 values are identical)."""
    torch = gpu
    from rtx_nerf_amd import api
    W, L, E = 128, 8, 112
    net = api.Network(n_neurons=W, n_hidden_layers=L)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(W, L, E, seed=9)))
    g = torch.Generator(device="cuda").manual_seed(S)
    enc = (torch.rand((E, S), device="cuda", generator=g) * 2 - 1).half()
    dout = ((torch.rand((S, 4), device="cuda", generator=g) - 0.5) * 0.02).half()
    dout[S // 3: S // 3 + 300_001] = 0
    n_params = E * W + (L - 1) * W * W + 16 * W

    def grads(a, b, dparams):
        n = b - a
        Sp = api.padded_samples(n)
        encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
        encT[:, :n] = enc[:, a:b]
        ws = net.train_workspace(n)
        out = net.train_forward(encT, n, ws)
        net.train_backward(encT, out, dout[a:b].contiguous(), n, ws, dparams)
        torch.cuda.synchronize()

    whole = torch.zeros(n_params, dtype=torch.float32, device="cuda")
    grads(0, S, whole)
    cuts = [0, 1, 70_001, S // 5, S // 3 + 77, S // 2, S - 300, S]
    parts = torch.zeros(n_params, dtype=torch.float32, device="cuda")
    for a, b in zip(cuts[:-1], cuts[1:]):
        grads(a, b, parts)
    scale = whole.abs().max().item()
    assert scale > 0 and torch.isfinite(whole).all()
    err = (whole - parts).abs().max().item()
    print(f"additivity: max |whole - parts| = {err:.3e}, largest entry {scale:.3e}")
    assert err <= 2e-5 * scale, (err, scale)        # measured: 1e-6


# ---------------------------------------------------------------------------------------------------- lean path (8 x 128)
def _lean_case(torch, api, n, seed=3, passes=None):
    rng = np.random.default_rng(seed)
    W, L, E = 128, 8, 112
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(W, L, E, seed=seed)))
    Sp = api.padded_samples(n)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    encT[:, :n] = _dev(torch, rng.uniform(-1, 1, (E, n)).astype(np.float16))
    return net, encT, Sp, rng


@pytest.mark.parametrize("n", [256, 700, 5000, 66_000, 300_000])   # 300,000: the three passes side by side in one launch
def test_lean_path_equals_the_saved_activation_path(gpu, oracle, n):
    """the 8 x 128 training backward WITHOUT materialised activations (rtxn_mlp_train_forward_lean: outputs
    + sign masks; rtxn_mlp_train_backward_lean: dgrad chain + weight gradient with the activations recomputed from the encoding
    in passes of three layers) against the saved-activation pair on the same inputs: identical outputs and masks (bit for bit: the same
    forward kernel), identical dZ (the same chain kernel on the same masks), weight gradients equal up to the summation order
    of fp32 accumulation -- the recomputed activations are the saved ones bit for bit, so the only difference is WHERE partial
    sums are rounded (per-block register accumulators + one atomic pass against per-chunk atomics): 2e-5 of the gradient's
    norm and 1e-4 of its largest element.  And against the oracle with the usual training tolerances.  The workspace is half the size."""
    torch = gpu
    from rtx_nerf_amd import api
    net, encT, Sp, rng = _lean_case(torch, api, n)
    assert net.lean_supported()
    W, L, E = 128, 8, 112
    ws = net.train_workspace(n)
    wl = net.train_lean_workspace(n)
    assert wl.numel() * 2 < 0.52 * ws.numel() * 2 and wl.numel() * 2 <= (L * W + 16 + 8 * L) * 2 * Sp + Sp // 256 + 64
    out = net.train_forward(encT, n, ws)
    out_l = net.train_forward_lean(encT, n, wl)
    torch.cuda.synchronize()
    assert torch.equal(out, out_l)
    masks = ws[(2 * L * W + 16) * Sp:(2 * L * W + 16 + 8 * L) * Sp]
    masks_l = wl[(L * W + 16) * Sp:(L * W + 16 + 8 * L) * Sp]
    assert torch.equal(masks.view(torch.int16), masks_l.view(torch.int16))
    dout = _dev(torch, (rng.standard_normal((n, 4)) * 0.05).astype(np.float16))
    dp = torch.zeros(net.n_params(), device="cuda")
    net.train_backward(encT, out, dout, n, ws, dp, None)
    dpl = torch.zeros(net.n_params(), device="cuda")
    net.train_backward_lean(encT, out_l, dout, n, wl, dpl)
    torch.cuda.synchronize()
    dz = ws[L * W * Sp:(2 * L * W + 16) * Sp]
    dz_l = wl[:(L * W + 16) * Sp]
    assert torch.equal(dz.view(torch.int16), dz_l.view(torch.int16))
    a, b = dp.cpu().numpy(), dpl.cpu().numpy()
    assert np.isfinite(b).all() and np.abs(a).max() > 0
    # per layer: a defect confined to one layer must not hide in the norm of the whole gradient
    off = 0
    for l in range(L + 1):
        M, N = (16 if l == L else W), (E if l == 0 else W)
        ga, gb = a[off:off + M * N], b[off:off + M * N]
        assert np.linalg.norm(ga) > 0
        assert np.linalg.norm(ga - gb) <= 2e-5 * np.linalg.norm(ga), f"layer {l}"
        assert np.abs(ga - gb).max() <= 1e-4 * np.abs(ga).max(), f"layer {l}"
        off += M * N
    assert off == a.size and np.all(b[-16 * W:].reshape(16, W)[4:] == 0)
    # the oracle, from the GPU's own forward state (as test_mlp_train_forward_and_backward)
    if n <= 5000:
        params = net.get_params().cpu().numpy() if hasattr(net, "get_params") else scenes.xavier_params_fp16(W, L, E, seed=3)
        enc = encT[:, :n].T.contiguous().cpu().numpy()
        acts = ws[:L * W * Sp].reshape(L, W, Sp).cpu().numpy()
        acts_sm = np.ascontiguousarray(np.transpose(acts[:, :, :n], (0, 2, 1)))
        want_dp, _ = oracle.mlpe_backward(W, L, 1, params, enc, acts_sm, out.cpu().numpy(), dout.cpu().numpy())
        assert np.linalg.norm(b - want_dp) < 2e-2 * np.linalg.norm(want_dp)
        assert np.abs(b - want_dp).max() < 3e-2 * np.abs(want_dp).max()
    # accumulate semantics
    net.train_backward_lean(encT, out_l, dout, n, wl, dpl)
    np.testing.assert_allclose(dpl.cpu().numpy(), 2 * b, rtol=1e-3, atol=1e-6 * np.abs(b).max() + 1e-9)


def test_lean_path_over_live_segments_and_dead_tiles(gpu):
    """The lean backward with a live list (only the listed segments are visited; dZ compact) and with tiles whose loss gradient
    is all zero (mlp_bwd_kernel writes no dZ for them: the weight-gradient kernel must step over them, also with no list)."""
    torch = gpu
    from rtx_nerf_amd import api
    P, K = 700, 32
    S = P * K
    net, encT, Sp, rng = _lean_case(torch, api, S, seed=5)
    wl = net.train_lean_workspace(S)
    wl.fill_(float("nan"))                       # whatever the kernels do not write must not be read
    out = net.train_forward_lean(encT, S, wl)
    ws = net.train_workspace(S)
    net.train_forward(encT, S, ws)
    live = np.zeros(P, bool)
    live[rng.choice(P, 90, replace=False)] = True
    live[[0, P - 1]] = True
    live[8:40] = False                           # four whole dead 256-sample tiles in the list-free run
    dout = np.zeros((P, K, 4), np.float16)
    dout[live] = (rng.standard_normal((int(live.sum()), K, 4)) * 0.05).astype(np.float16)
    dout_d = _dev(torch, dout.reshape(S, 4))
    want = torch.zeros(net.n_params(), device="cuda")
    net.train_backward(encT, out, dout_d, S, ws, want, None)
    got = torch.zeros(net.n_params(), device="cuda")
    net.train_backward_lean(encT, out, dout_d, S, wl, got)                 # no list: dead tiles skipped by their flags
    lws = api.live_segments_workspace(P)
    api.live_segments(dout_d, P, P, lws)
    assert int(lws[0].item()) == int(live.sum())
    wl2 = net.train_lean_workspace(S)
    wl2.fill_(float("nan"))
    out2 = net.train_forward_lean(encT, S, wl2)
    got_live = torch.zeros(net.n_params(), device="cuda")
    net.train_backward_lean(encT, out2, dout_d, S, wl2, got_live, live_ws=lws)
    torch.cuda.synchronize()
    for g in (got, got_live):
        assert bool(torch.isfinite(g).all()) and float(want.norm()) > 0
        assert float((g - want).norm()) <= 2e-5 * float(want.norm())


def test_lean_path_is_refused_for_other_models(gpu):
    torch = gpu
    from rtx_nerf_amd import api, _lib
    net = api.Network(n_neurons=128, n_hidden_layers=3, n_encoded_features=48)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(128, 3, 48, seed=1)))
    assert not net.lean_supported()
    assert _lib.lib().rtxn_mlp_train_lean_workspace_bytes(net._h, 1000) == 0
    encT = torch.zeros((48, 1024), dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.RtxnError, match="lean path"):
        net.train_forward_lean(encT, 1000, torch.zeros(16, dtype=torch.float16, device="cuda"))


@pytest.mark.parametrize("P,stype", [(1, 0), (7, 3), (8, 0), (9, 3), (300, 0), (5000, 3)])   # 0: REGULAR, 3: MIDPOINT_WORLD
def test_lean_forward_with_the_encoder_folded_in_equals_the_staged_pair(gpu, P, stype):
    """rtxn_mlp_train_forward_lean_segments (round 4: sampler + Composite-Frequency(3 x 10, 2 x 12) encoder inside the forward kernel,
    straight into layer 0's operands) against rtxn_encode_frequency_segments + rtxn_mlp_train_forward_lean on the same packed
    segments: outputs, radiance and the sign masks BIT FOR BIT (the same sin_turns arithmetic, one rounding to fp16, the same sums in
    the same order), for both deterministic sample types, ragged tiles included; a model with another encoding is refused."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(100 + P)
    W, L = 128, 8
    net = api.Network(n_neurons=W, n_hidden_layers=L)
    assert net.encoded_width() == 112 and net.lean_supported() and net.lean_fused_supported()
    net.set_params(_dev(torch, scenes.xavier_params_fp16(W, L, 112, seed=5)))
    start = _dev(torch, rng.uniform(-1, 1, (P, 3)).astype(np.float32))
    end = _dev(torch, (start.cpu().numpy() + rng.uniform(-0.2, 0.2, (P, 3))).astype(np.float32))
    view = _dev(torch, rng.uniform(0, 3.0, (P, 2)).astype(np.float32))
    n = P * 32
    Sp = api.padded_samples(n)
    encT = torch.full((112, Sp), 9.0, dtype=torch.float16, device="cuda")
    net.encode_frequency_segments(start, end, view, P, stype, encT)
    wa, wb = net.train_lean_workspace(n), net.train_lean_workspace(n)
    wa.zero_(); wb.zero_()
    oa = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
    ob = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
    ra = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    rb = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    net.train_forward_lean(encT, n, wa, oa, ra)
    net.train_forward_lean_segments(start, end, view, P, stype, wb, ob, rb)
    torch.cuda.synchronize()
    assert torch.equal(oa[:, :4], ob[:, :4]) and torch.equal(ra, rb)
    lo = (L * W + 16) * Sp                                  # the masks: u64[L][Sp][2] behind dZ and dZ_L
    ma, mb = wa[lo:lo + 8 * L * Sp].view(torch.int16), wb[lo:lo + 8 * L * Sp].view(torch.int16)     # bit patterns, not halves (NaNs)
    assert torch.equal(ma, mb) and bool((ma != 0).any())
    other = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=112)
    assert other.lean_supported() and not other.lean_fused_supported()
    with pytest.raises(api._lib.RtxnError):
        other.train_forward_lean_segments(start, end, view, P, stype, wb, ob)


@pytest.mark.parametrize("P,stype,live", [(9, 0, False), (300, 3, False), (2500, 0, True), (9000, 3, False), (9000, 0, True)])
def test_lean_backward_recomputing_the_encoding_equals_the_one_reading_it(gpu, P, stype, live):
    """rtxn_mlp_train_backward_lean_segments (the weight gradient recomputes the ENCODING with the activations: a column tile's
    segment constants through the scalar cache, encode_freq_fragments_3_10_2_12) against rtxn_mlp_train_backward_lean on the encT
    the standalone encoder wrote for the same segments: the same operands bit for bit, so the gradients agree to the order of the fp32
    atomic adds (2e-5 of the norm).  One launch per pass (small batches) and the three passes side by side (9,000 segments); with
    spans of zero loss gradient and the live list."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(300 + P)
    W, L = 128, 8
    net = api.Network(n_neurons=W, n_hidden_layers=L)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(W, L, 112, seed=6)))
    start = _dev(torch, rng.uniform(-1, 1, (P, 3)).astype(np.float32))
    end = _dev(torch, (start.cpu().numpy() + rng.uniform(-0.2, 0.2, (P, 3))).astype(np.float32))
    view = _dev(torch, rng.uniform(0, 3.0, (P, 2)).astype(np.float32))
    n = P * 32
    Sp = api.padded_samples(n)
    encT = torch.zeros((112, Sp), dtype=torch.float16, device="cuda")
    net.encode_frequency_segments(start, end, view, P, stype, encT)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    lws = None
    if live:
        seg_dead = rng.random(P) < 0.6
        dout.reshape(P, 32, 4)[seg_dead] = 0
        lws = api.live_segments_workspace(P)
    dout_d = _dev(torch, dout)
    if live:
        api.live_segments(dout_d, P, P, lws)
    res = []
    for fused in (False, True):
        ws = net.train_lean_workspace(n)
        out = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
        dp = torch.zeros(net.n_params(), dtype=torch.float32, device="cuda")
        if fused:
            net.train_forward_lean_segments(start, end, view, P, stype, ws, out)
            net.train_backward_lean_segments(start, end, view, P, stype, out, dout_d, ws, dp, live_ws=lws)
        else:
            net.train_forward_lean(encT, n, ws, out)
            net.train_backward_lean(encT, out, dout_d, n, ws, dp, live_ws=lws)
        torch.cuda.synchronize()
        res.append(dp.double().cpu().numpy())
    a, b = res
    assert np.isfinite(b).all() and np.linalg.norm(a) > 0
    assert np.linalg.norm(a - b) <= 2e-5 * np.linalg.norm(a) and np.abs(a - b).max() <= 1e-4 * np.abs(a).max()


@pytest.mark.parametrize("act", [0, 1])
def test_lean_gradients_match_torch_autograd(gpu, act):
    """A reference that is neither this repository's oracle nor its kernels: the 8 x 128 model rebuilt as float64 torch modules on the
    CPU (weights = the fp16 parameters exactly, tcnn layout: layer l is [out][in] row-major, the output layer 16 x 128), the same
    encoded inputs, loss = sum(output[:, :4] * g), gradients by torch.autograd -- against the lean path (encT form and the form with
    sampler + encoder folded in) fed g as dL/d(output).  fp16 activations against float64: 3e-3 of the gradient's norm for the output
    layer, 6e-2 for the hidden ones (measured 7e-4 and 1.5e-2 ... 4.5e-2, growing with depth); outputs 2e-2 absolute."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(77 + act)
    W, L, E, P = 128, 8, 112, 96
    n = P * 32
    net = api.Network(n_neurons=W, n_hidden_layers=L, output_activation=act)
    params = scenes.xavier_params_fp16(W, L, E, seed=9)
    net.set_params(_dev(torch, params))
    start = _dev(torch, rng.uniform(-1, 1, (P, 3)).astype(np.float32))
    end = _dev(torch, (start.cpu().numpy() + rng.uniform(-0.2, 0.2, (P, 3))).astype(np.float32))
    view = _dev(torch, rng.uniform(0, 3.0, (P, 2)).astype(np.float32))
    Sp = api.padded_samples(n)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    net.encode_frequency_segments(start, end, view, P, 0, encT)
    g = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    g_d = _dev(torch, g)

    # ---- torch, float64, CPU ----
    x = encT[:, :n].t().contiguous().cpu().double()
    sizes = [(W, E)] + [(W, W)] * (L - 1) + [(16, W)]
    ws, off = [], 0
    for o, i in sizes:
        ws.append(torch.from_numpy(params[off:off + o * i].astype(np.float64).reshape(o, i)).requires_grad_(True))
        off += o * i
    assert off == params.size
    h = x
    for w in ws[:-1]:
        h = torch.relu(h @ w.t())
    z = h @ ws[-1].t()
    y = torch.sigmoid(z) if act else z
    (y[:, :4] * torch.from_numpy(g.astype(np.float64))).sum().backward()
    want = np.concatenate([w.grad.numpy().reshape(-1) for w in ws])
    want_out = y.detach().numpy()[:, :4]

    for folded in (False, True):
        wsp = net.train_lean_workspace(n)
        out = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
        dp = torch.zeros(net.n_params(), dtype=torch.float32, device="cuda")
        if folded:
            net.train_forward_lean_segments(start, end, view, P, 0, wsp, out)
            net.train_backward_lean_segments(start, end, view, P, 0, out, g_d, wsp, dp)
        else:
            net.train_forward_lean(encT, n, wsp, out)
            net.train_backward_lean(encT, out, g_d, n, wsp, dp)
        torch.cuda.synchronize()
        assert np.abs(out[:, :4].float().cpu().numpy() - want_out).max() <= 2e-2
        got = dp.double().cpu().numpy()
        off = 0
        errs = []
        for k, (o, i) in enumerate(sizes):
            a, b = got[off:off + o * i], want[off:off + o * i]
            if k == len(sizes) - 1:                       # rows 4..15 of the output layer carry no loss
                a, b = a[:4 * W], b[:4 * W]
                assert np.abs(got[off + 4 * W:off + o * i]).max() == 0.0
            errs.append(np.linalg.norm(a - b) / np.linalg.norm(b))
            off += o * i
        # measured: output layer 7e-4, layer 7 1.5e-2, ... layer 0 4.5e-2 of the norm -- half-precision activations and dZ (as tcnn keeps
        # them) and the ReLU masks of activations within an fp16 rounding of zero, compounding layer by layer against a float64 chain;
        # a wrong layout, transposition or sign would be O(1)
        assert errs[-1] <= 3e-3 and max(errs[:-1]) <= 6e-2, (folded, ["%.2e" % e for e in errs])


def test_hash_scatter_is_the_adjoint_of_the_encoder_at_the_bench_size(gpu):
    """A size-independent property at BASELINE configs[2]'s own size (L = 16, F = 2, T = 2^19, base 16 x 1.5; 660 k samples), no oracle
    involved: the encoding is linear in the table, so for any table t and any d, <encode(t), d> = <t, scatter(d)>.  The encoder is
    held to tiny-cuda-nn's published formulas by tests/golden/kat_north_star.npz; this identity then pins the scatter -- every level,
    the fp32 form and the mixed form (hashed levels through packed fp16 atomics).  fp16 rounding of the encoding and (mixed) of the
    gradient entries: 2e-3 / 3e-3 relative."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(2026)
    n = 660_000
    hg = api.HashGrid(16, 2, 19, 16, 1.5, n_dir_freqs=4)
    nh = 32
    x = _dev(torch, np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0, 3, (n, 2))], axis=1).astype(np.float32))
    table = _dev(torch, (rng.standard_normal(hg.n_params()) * 0.5).astype(np.float16))
    E, Sp = hg.encoded_width(), api.padded_samples(n)
    enc = hg.encode(table, x)                                      # half[E][Sp]
    d = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    d[:nh, :n] = _dev(torch, (rng.standard_normal((nh, n)) * 0.25).astype(np.float16))     # nothing on the direction features: not the table's
    lhs = float((enc[:nh, :n].double() * d[:nh, :n].double()).sum())
    g32 = torch.zeros(hg.n_params(), device="cuda")
    hg.backward(x, d, g32)
    rhs = float((table.double() * g32.double()).sum())
    scale = float((enc[:nh, :n].double() * d[:nh, :n].double()).abs().sum())
    assert abs(lhs) > 1e-6 * scale and abs(lhs - rhs) <= 2e-3 * scale ** 0.5 * abs(lhs) ** 0.5 + 2e-4 * abs(lhs), (lhs, rhs)
    lo = hg.hashed_offset()
    m32 = torch.zeros(hg.n_params(), device="cuda")
    m16 = torch.zeros(hg.n_params() - lo, dtype=torch.float16, device="cuda")
    hg.backward_mixed(x, d, m32, m16)
    rhs_m = float((table[:lo].double() * m32[:lo].double()).sum() + (table[lo:].double() * m16.double()).sum())
    assert abs(lhs - rhs_m) <= 3e-3 * scale ** 0.5 * abs(lhs) ** 0.5 + 3e-3 * abs(lhs), (lhs, rhs_m)
    # level by level too (a level with its gradient in the wrong place would cancel nowhere)
    offs = [hg.level_offset(l) for l in range(17)]                  # in parameters (entries x features)
    for l in range(16):
        a = float((enc[2 * l:2 * l + 2, :n].double() * d[2 * l:2 * l + 2, :n].double()).sum())
        b = float((table[offs[l]:offs[l + 1]].double() * g32[offs[l]:offs[l + 1]].double()).sum())
        s = float((enc[2 * l:2 * l + 2, :n].double() * d[2 * l:2 * l + 2, :n].double()).abs().sum())
        assert abs(a - b) <= 5e-3 * s ** 0.5 * max(abs(a), 1.0) ** 0.5 + 1e-3 * abs(a), (l, a, b)
