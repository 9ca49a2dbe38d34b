"""Deterministic mode (rtxn_set_deterministic_workspace) against float64 references, element by element, and against the default
float-atomic mode.  The bit-identity tests of tests/test_gpu_training_loop.py say that the mode is reproducible; these say that
what it reproduces is the gradient: the hash scatter (every form), the saved-activation, recompute and lean weight gradients,
whole batches through rtxn_train_gradients, non-finite and out-of-range contributions, and a Trainer that dies while its shadows
are registered.

Notation of the bounds: u = 2^-24 (fp32 unit roundoff).  The fixed point holds value x 2^40, so each atomic contribution is
rounded once to 2^-40 (error <= 2^-41), and the fold rounds the exact integer sum once to fp32 (<= u relative)."""
import gc

import numpy as np
import pytest

from rtx_nerf_amd import scenes

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# Hash scatter, fp32 form.  A contribution is w * d with the kernel's own fp32 trilinear weight w (oracle: (double)w * d exactly):
# one fp32 product rounding (1 u), then the wave's run sum: a segmented scan of four row steps (row_shr 1, 2, 4, 8) and up to three
# row carries -- at most 7 fp32 additions on the path of any term (7 u), so |run sum - exact| <= 8 u * sum|contributions|.
# Every run sum is one atomic (<= 2^-41 each; at most 8 per sample and entry: N_CONTRIB = 8 S bounds the count), the fold one
# fp32 rounding, and the oracle returns its double sum rounded to fp32 once more: 2 u |want|.
# Measured on the MI355X: max |err| / bound 0.17 over the three grids and all forms.
C_SCATTER = 8


def _scatter_bound(want, A, n_contrib):
    return 2 * U * np.abs(want) + C_SCATTER * U * A + n_contrib * 2.0 ** -41


# Saved-activation weight gradients dW = dZ X^T, restated in float64 from the kernel's own fp16 dZ and X: only the fp32 summation
# is left.  A workgroup sums its chunk of at most 4 x 1024 samples in MFMA k-steps of at least 8 (<= 512 dependent fp32 adds),
# then the <= ceil(n / 4096) partials meet (float atomics or the fixed point), then the fold: k = 512 + ceil(n / 4096) + 2.
# Measured on the MI355X: max |err| / (k u |dZ| |X|^T) 1.4e-3 ... 1.1e-2 over the shapes below, both modes.
def _k_wgrad(n):
    return 512 + -(-n // 4096) + 2


# Deterministic against default weight gradients, per layer: the same per-workgroup partials summed in another order (fp32
# atomics against exact integer sums), 1e-5 of the layer's norm.  Measured on the MI355X: 0 ... 4.9e-7 over every test here.
DET_VS_DEFAULT = 1e-5


@pytest.fixture(autouse=True)
def _restore_default_mode(gpu):
    yield
    from rtx_nerf_amd import api
    api.set_deterministic(None, None)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shadows(api, n_mlp=0, n_table=0):
    m = api.deterministic_shadow(n_mlp) if n_mlp else None
    t = api.deterministic_shadow(n_table) if n_table else None
    api.set_deterministic(m, t)
    return m, t


def _segments(torch, api, rng, P, stype):
    """P one-segment rays of 32 samples; the sampler's own positions (what the *_segments forms recompute bit for bit)."""
    sp = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    ep = (sp + rng.uniform(-0.06, 0.06, (P, 3))).astype(np.float32)
    sv = np.stack([rng.uniform(0, 3.1, P), rng.uniform(-3.1, 3.1, P)], 1).astype(np.float32)
    sp_d, ep_d, sv_d = _dev(torch, sp), _dev(torch, ep), _dev(torch, sv)
    S = 32 * P
    samples = torch.zeros((S, 5), device="cuda")
    t = torch.zeros(S, device="cuda")
    api.launchSampler(sp_d, ep_d, sv_d, t, samples, P, 8, _dev(torch, np.ones(P, np.int32)), _dev(torch, np.arange(P, dtype=np.int32)), stype)
    return sp_d, ep_d, sv_d, samples


# --------------------------------------------------------------------------------------------------------------- A.1 scatter
@pytest.mark.parametrize("levels,feat,log2,base,scale,P", [(16, 2, 19, 16, 1.5, 19_000), (4, 2, 10, 4, 1.7, 400), (8, 4, 14, 8, 2.0, 3000),
                                                                   (5, 1, 10, 4, 1.7, 300), (2, 8, 12, 8, 2.0, 300)])
def test_deterministic_hash_scatter_matches_float64(gpu, oracle, levels, feat, log2, base, scale, P):
    """The deterministic scatter (hashgrid_backward_kernel<false, true> + det_fold_kernel) per element against the oracle's double
    sum, in every form: HashGrid.backward, backward_mixed (hashed levels folded into fp16), backward_segments (REGULAR and
    MIDPOINT_WORLD) and the live-list form; accumulate semantics into pre-filled buffers; three calls bit-identical; shadows clean.
    The largest grid runs 608 k samples so that both the dense and the hashed levels see real traffic.  The segments reach a
    little past [-1, 1]: cells at g = -1 once shared one wave run whatever their second coordinate (the run key packed g0 | g1 << 16)
    and both modes sent those sums to the wrong entries."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(levels * 7 + feat)
    hg = api.HashGrid(levels, feat, log2, base, scale, n_dir_freqs=4)
    ocfg = oracle.hg_cfg(levels, feat, log2, base, scale)
    NP, E, nh = hg.n_params(), hg.encoded_width(), levels * feat
    S = 32 * P
    Sp = api.padded_samples(S)
    live = rng.random(P) < 0.7
    live[[0, P - 1]] = True
    for stype in (0, 3):
        sp_d, ep_d, sv_d, samples = _segments(torch, api, np.random.default_rng(stype + 1), P, stype)
        denc = np.zeros((E, Sp), np.float16)
        denc[:nh, :S] = (rng.standard_normal((nh, S)) * 0.5).astype(np.float16)
        denc[:nh, :S].reshape(nh, P, 32)[:, ~live] = 0             # dead segments carry no gradient (the live form skips them)
        denc_d = _dev(torch, denc)
        x = samples.cpu().numpy()
        dT = denc[:, :S].T.copy()
        want = oracle.hg_backward(ocfg, x, dT).astype(np.float64)
        A = oracle.hg_backward(ocfg, x, np.abs(dT)).astype(np.float64) * (1 + 4 * U)
        assert np.count_nonzero(want) > 0
        bound = _scatter_bound(want, A, 8 * S)

        def run(form, pre32=None, pre16=None, half=False):
            lo = hg.hashed_offset()
            d32 = pre32.clone() if pre32 is not None else torch.zeros(NP, device="cuda")
            d16 = None
            if half:
                d16 = pre16.clone() if pre16 is not None else torch.zeros(NP - lo, dtype=torch.float16, device="cuda")
            if form == "plain":
                (hg.backward_mixed(samples, denc_d, d32, d16) if half else hg.backward(samples, denc_d, d32))
            elif form == "segments":
                hg.backward_segments(sp_d, ep_d, P, stype, denc_d, d32, d16)
            else:
                dout = torch.zeros((S, 4), dtype=torch.float16, device="cuda")
                dout.view(P, 32, 4)[torch.from_numpy(live).cuda(), 0, 0] = 1.0
                ws = api.live_segments_workspace(P)
                api.live_segments(dout, P, P, ws)
                hg.backward_segments(sp_d, ep_d, P, stype, denc_d, d32, d16, live_ws=ws)
            torch.cuda.synchronize()
            return d32, d16

        forms = ("plain", "segments", "live") if stype == 0 else ("segments",)
        for form in forms:
            m, t = _shadows(api, n_table=NP)
            got = [run(form)[0] for _ in range(3)]
            assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]), f"{form}: repeated calls differ"
            g = got[0].double().cpu().numpy()
            err = np.abs(g - want)
            _measured(f"scatter {levels}x{feat} {form} err / bound", float((err / bound).max()))
            assert np.all(err <= bound), (form, stype, float((err / bound).max()), int((err > bound).sum()))
            # accumulate semantics: the fold adds to what the buffer holds, one rounding
            pre = _dev(torch, rng.standard_normal(NP).astype(np.float32))
            acc, _ = run(form, pre32=pre)
            assert torch.equal(acc, pre + got[0]), f"{form}: pre-filled buffer"
            if feat == 2:
                lo = hg.hashed_offset()
                h32, h16 = run(form, half=True)
                assert torch.equal(h32[:lo], got[0][:lo]) and bool((h32[lo:] == 0).all())
                # each hashed fp16 entry is the fp16 rounding of the deterministic fp32 value
                assert torch.equal(h16, got[0][lo:].half()), f"{form}: hashed fp16 entries"
                pre16 = (torch.randn(NP - lo, device="cuda") * 0.5).half()
                a32, a16 = run(form, pre32=pre, pre16=pre16, half=True)
                assert torch.equal(a16, (pre16.float() + got[0][lo:]).half()) and torch.equal(a32[:lo], (pre + got[0])[:lo])
                if lo < NP:
                    # the default mixed form at its own bars (tests/test_gpu_train.py), and the deterministic fp16 error no larger
                    api.set_deterministic(None, None)
                    d32, d16 = run(form, half=True)
                    ref = want[lo:]
                    e_def = d16.double().cpu().numpy() - ref
                    e_det = h16.double().cpu().numpy() - ref
                    assert np.abs(e_def).max() < 1e-2 * max(1.0, np.abs(ref).max())
                    assert np.linalg.norm(e_def) < 1e-3 * np.linalg.norm(ref)
                    assert np.linalg.norm(e_det) <= np.linalg.norm(e_def), (np.linalg.norm(e_det), np.linalg.norm(e_def))
                    assert np.all(np.abs(d32.double().cpu().numpy()[:lo] - want[:lo]) <= 1e-4 * max(1.0, np.abs(want).max()))
            assert int(t.abs().max()) == 0, f"{form}: shadow left non-zero"
            api.set_deterministic(None, None)


# ------------------------------------------------------------------------------------------ A.2 saved-activation weight gradients
@pytest.mark.parametrize("W,L,E,n", [(64, 1, 48, 3000), (64, 2, 112, 5000), (64, 4, 176, 4100), (128, 1, 112, 2049),
                                     (128, 2, 48, 6000), (128, 4, 144, 3000)])
def test_saved_activation_weight_gradients_match_float64(gpu, W, L, E, n):
    """train_forward + train_backward (wgrad_lds_kernel / wgrad_kernel, the 16 x W output layer included), both modes, against
    dW_l = dZ_l X_l^T restated in float64 from the kernel's OWN fp16 tensors in the workspace (acts | dz | dzL, X_0 = encT)."""
    torch = gpu
    from rtx_nerf_amd import api
    rng = np.random.default_rng(W * 10 + L + E)
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E, output_activation=1)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(W, L, E, seed=L + E)))
    Sp = api.padded_samples(n)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    encT[:, :n] = _dev(torch, rng.uniform(-1, 1, (E, n)).astype(np.float16))
    dout = _dev(torch, (rng.standard_normal((n, 4)) * 0.05).astype(np.float16))
    res = {}
    for det in (False, True):
        if det:
            m, _ = _shadows(api, n_mlp=net.n_params())
        ws = net.train_workspace(n)
        out = net.train_forward(encT, n, ws)
        dp = torch.zeros(net.n_params(), device="cuda")
        net.train_backward(encT, out, dout, n, ws, dp)
        torch.cuda.synchronize()
        acts = ws[:L * W * Sp].view(L, W, Sp)[:, :, :n].double()
        dz = ws[L * W * Sp:2 * L * W * Sp].view(L, W, Sp)[:, :, :n].double()
        dzL = ws[2 * L * W * Sp:2 * L * W * Sp + 16 * Sp].view(16, Sp)[:, :n].double()
        X = [encT[:, :n].double()] + [acts[l] for l in range(L)]
        dZ = [dz[l] for l in range(L)] + [dzL]
        ref = torch.cat([(a @ x.t()).reshape(-1) for a, x in zip(dZ, X)])
        mag = torch.cat([(a.abs() @ x.abs().t()).reshape(-1) for a, x in zip(dZ, X)])
        got = dp.double()
        err = (got - ref).abs()
        bound = U * ref.abs() + _k_wgrad(n) * U * mag
        assert float(ref.abs().max()) > 0 and bool(torch.isfinite(got).all())
        _measured(f"wgrad {W}x{L} E{E} det={det} err / (k u |dZ||X|)", float((err / (_k_wgrad(n) * U * mag).clamp_min(1e-30)).max()))
        assert bool((err <= bound).all()), (det, float((err / bound.clamp_min(1e-30)).max()))
        res[det] = got
        if det:
            assert int(m.abs().max()) == 0
            api.set_deterministic(None, None)
    _per_layer_close(res[False], res[True], [W * E] + [W * W] * (L - 1) + [16 * W])


def _measured(what, value):
    print(f"measured {what}: {value:.3e}")


def _per_layer_close(a, b, sizes, tol=DET_VS_DEFAULT):
    off = 0
    for k, s in enumerate(sizes):
        x, y = a[off:off + s], b[off:off + s]
        _measured("det vs default, layer norm", float((x - y).norm() / x.norm()))
        assert float((x - y).norm()) <= tol * float(x.norm()) + 1e-30, (k, float((x - y).norm() / x.norm()))
        off += s


# ------------------------------------------------------------------------------------------------- A.3 recompute and lean paths
def _autograd(torch, params, sizes, x, g, act):
    """float64 autograd of sum(output[:, :4] * g) for the tcnn-layout MLP (layer l: [out][in] row-major), on the GPU."""
    ws, off = [], 0
    for o, i in sizes:
        ws.append(torch.from_numpy(params[off:off + o * i].astype(np.float64).reshape(o, i)).cuda().requires_grad_(True))
        off += o * i
    h = x.double()
    for w in ws[:-1]:
        h = torch.relu(h @ w.t())
    z = h @ ws[-1].t()
    y = torch.sigmoid(z) if act else z
    (y[:, :4] * g.double()).sum().backward()
    return torch.cat([w.grad.reshape(-1) for w in ws])


def _layer_errors(got, want, sizes, W):
    errs, off = [], 0
    for k, (o, i) in enumerate(sizes):
        a, b = got[off:off + o * i], want[off:off + o * i]
        if k == len(sizes) - 1:
            assert float(a[4 * W:].abs().max()) == 0.0
            a, b = a[:4 * W], b[:4 * W]
        errs.append(float((a - b).norm() / b.norm()))
        off += o * i
    return errs


@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("E", [16, 32, 48, 64])
def test_recompute_path_both_modes_match_autograd(gpu, L, E):
    """mlp_bwd_fused64_kernel (every KS0 = E / 16), and its live form, in both modes: against float64 autograd at the bars of
    tests/test_gpu_train.py::test_lean_gradients_match_torch_autograd, and deterministic against default per layer."""
    torch = gpu
    from rtx_nerf_amd import api
    W, P = 64, 120
    n = 32 * P
    rng = np.random.default_rng(L * 100 + E)
    params = scenes.xavier_params_fp16(W, L, E, seed=E + L)
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E, output_activation=1)
    net.set_params(_dev(torch, params))
    assert net.recompute_supported()
    Sp = api.padded_samples(n)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    encT[:, :n] = _dev(torch, rng.uniform(-1, 1, (E, n)).astype(np.float16))
    g = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    g.reshape(P, 32, 4)[rng.random(P) < 0.4] = 0
    g_d = _dev(torch, g)
    sizes = [(W, E)] + [(W, W)] * (L - 1) + [(16, W)]
    want = _autograd(torch, params, sizes, encT[:, :n].t(), g_d, 1)
    lws = api.live_segments_workspace(P)
    api.live_segments(g_d, P, P, lws)
    res = {}
    for det in (False, True):
        for live in (False, True):
            if det:
                _shadows(api, n_mlp=net.n_params())
            out = net.train_forward_outputs(encT, n)
            dp = torch.zeros(net.n_params(), device="cuda")
            if live:
                net.train_backward_recompute_live(encT, out, g_d, n, lws, dp)
            else:
                net.train_backward_recompute(encT, out, g_d, n, dp)
            torch.cuda.synchronize()
            api.set_deterministic(None, None)
            errs = _layer_errors(dp.double(), want, sizes, W)
            assert errs[-1] <= 3e-3 and max(errs[:-1]) <= 6e-2, (det, live, ["%.2e" % e for e in errs])
            res[det, live] = dp.double()
    flat = [s[0] * s[1] for s in sizes]
    _per_layer_close(res[False, False], res[True, False], flat)
    _per_layer_close(res[False, True], res[True, True], flat)


@pytest.mark.parametrize("n", [700, 66_000, 300_000])
def test_lean_path_both_modes_match_autograd(gpu, n):
    """The 8 x 128 lean path (wgrad_recompute_kernel*, and at 300 k samples the single-launch wgrad_recompute_all_kernel), encT and
    segment forms and the live list, in both modes: against float64 autograd at the bars of
    test_lean_gradients_match_torch_autograd, deterministic against default per layer."""
    torch = gpu
    from rtx_nerf_amd import api
    W, L, E = 128, 8, 112
    P = -(-n // 32)
    rng = np.random.default_rng(n)
    params = scenes.xavier_params_fp16(W, L, E, seed=9)
    net = api.Network(n_neurons=W, n_hidden_layers=L)
    net.set_params(_dev(torch, params))
    assert net.lean_supported() and net.lean_fused_supported()
    start = _dev(torch, rng.uniform(-1, 1, (P, 3)).astype(np.float32))
    end = _dev(torch, (start.cpu().numpy() + rng.uniform(-0.2, 0.2, (P, 3))).astype(np.float32))
    view = _dev(torch, rng.uniform(0, 3.0, (P, 2)).astype(np.float32))
    S = 32 * P
    Sp = api.padded_samples(S)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    net.encode_frequency_segments(start, end, view, P, 0, encT)
    g = (rng.standard_normal((S, 4)) * 0.05).astype(np.float16)
    g[n:] = 0                                                    # the encT form covers n samples, the segment form all of P
    g.reshape(P, 32, 4)[rng.random(P) < 0.3] = 0
    g_d = _dev(torch, g)
    sizes = [(W, E)] + [(W, W)] * (L - 1) + [(16, W)]
    want = _autograd(torch, params, sizes, encT[:, :S].t(), g_d, 1)
    lws = api.live_segments_workspace(P)
    api.live_segments(g_d, P, P, lws)
    flat = [s[0] * s[1] for s in sizes]
    for form in ("encT", "segments", "live"):
        res = {}
        for det in (False, True):
            if det:
                _shadows(api, n_mlp=net.n_params())
            ws = net.train_lean_workspace(S)
            out = torch.zeros((S, 16), dtype=torch.float16, device="cuda")
            dp = torch.zeros(net.n_params(), device="cuda")
            if form == "segments":
                net.train_forward_lean_segments(start, end, view, P, 0, ws, out)
                net.train_backward_lean_segments(start, end, view, P, 0, out, g_d, ws, dp)
            else:
                m = n if form == "encT" else S
                net.train_forward_lean(encT, m, ws, out)
                net.train_backward_lean(encT, out, g_d, m, ws, dp, live_ws=lws if form == "live" else None)
            torch.cuda.synchronize()
            api.set_deterministic(None, None)
            errs = _layer_errors(dp.double(), want, sizes, W)
            assert errs[-1] <= 3e-3 and max(errs[:-1]) <= 6e-2, (form, det, ["%.2e" % e for e in errs])
            res[det] = dp.double()
        _per_layer_close(res[False], res[True], flat)


# ------------------------------------------------------------------------------------------------------------- A.4 whole batch
def _small_trainer(torch, encoding, mode, neurons, layers, **kw):
    from rtx_nerf_amd.train import Trainer
    R, B = 16, 900
    occ = torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, 0.75)).view(np.int32).copy()).cuda()
    hgd = dict(n_levels=8, n_features=2, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.6)
    return Trainer(R, occ, encoding=encoding, n_neurons=neurons, n_hidden_layers=layers, hashgrid=hgd if encoding == "hash" else None,
                   n_dir_freqs=4, batch_rays=B, max_segments=B * 30, lr=1e-2, loss_scale=128.0,
                   density_scale=120.0 if mode == "nerf" else 1.0, mode=mode, seed=3, **kw)


def _batch(torch):
    from rtx_nerf_amd.train import camera_rays
    o, d = camera_rays(scenes.pose_spherical(40.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 30, 30)
    t = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (900, 3)).astype(np.float32)).cuda()
    return o, d, t


def _train_gradients(torch, tr, api, targets):
    """rtxn_train_gradients over the trainer's buffers and the segments its last traversal left (the count read on the device)."""
    n = targets.shape[0]
    hash_ = tr.encoding == "hash"
    tr.dparams.zero_()
    if hash_:
        tr.dtable.zero_()
        if tr.dtable_h is not None:
            tr.dtable_h.zero_()
    api.train_gradients(tr.net, grid=tr.hg if hash_ else None, n_dir_freqs=tr.hg.n_dir_freqs if hash_ else 0,
                        table=tr.table if hash_ else None, start_points=tr.start, end_points=tr.end, seg_view=tr.seg_view,
                        num_stored=tr.num_stored, indices=tr.indices, total_segments=tr.total, segment_capacity=tr.max_segments,
                        n_rays=n, sample_type=tr._stype(), t_scale=tr.density_scale if tr.mode == "nerf" else 1.0,
                        vr_mode=api.VR_NERF if tr.mode == "nerf" else api.VR_COMPAT, targets=targets,
                        loss_scale=tr.loss_scale, encT=tr.encT, dencT=tr.dencT, workspace=tr.ws, output_half=tr.out,
                        radiance=tr.radiance, t_vals=tr.t_vals, radiance_gradients=tr.dout, pixels=tr.pixels,
                        loss_gradients=tr.loss_grads, loss_sum=tr.loss, dparams=tr.dparams,
                        dtable=tr.dtable if hash_ else None, dtable_hashed_half=tr.dtable_h if (hash_ and tr.hash_fp16) else None,
                        live_ws=tr.live_ws if tr.live_segments else None, workspace_lean=tr.lean)
    torch.cuda.synchronize()
    out = [tr.dparams.double().clone()]
    if hash_:
        out += [tr.dtable.double().clone(), tr.dtable_h.double().clone() if tr.dtable_h is not None else None]
    return out


@pytest.mark.parametrize("encoding,mode,neurons,layers", [("hash", "nerf", 64, 4), ("freq", "nerf", 128, 8), ("freq", "compat", 128, 2)])
def test_whole_batch_gradients_agree_between_modes(gpu, encoding, mode, neurons, layers):
    """api.train_gradients (sampler ... backward with the count on the device) in both modes on one batch: dparams and the fp32
    table part agree per layer and level to DET_VS_DEFAULT, the hashed fp16 part at the fp16 bar of tests/test_gpu_train.py."""
    torch = gpu
    from rtx_nerf_amd import api
    tr = _small_trainer(torch, encoding, mode, neurons, layers)
    o, d, t = _batch(torch)
    tr.gradients(o, d, t)                   # the traversal's segments (and a first backward) in the trainer's buffers
    a = _train_gradients(torch, tr, api, t)
    _shadows(api, n_mlp=tr.master.numel(), n_table=tr.table_master.numel() if encoding == "hash" else 0)
    b = _train_gradients(torch, tr, api, t)
    api.set_deterministic(None, None)
    assert float(a[0].norm()) > 0
    W, L, E = neurons, layers, tr.net.encoded_width()
    _per_layer_close(a[0], b[0], [W * E] + [W * W] * (L - 1) + [16 * W])
    if encoding == "hash":
        hg, lo = tr.hg, tr.hashed_lo
        levels = [hg.level_offset(l) for l in range(hg.cfg.n_levels + 1)]
        fp32_levels = [(levels[l], levels[l + 1]) for l in range(hg.cfg.n_levels) if levels[l + 1] <= lo or b[2] is None]
        assert fp32_levels
        for s, e in fp32_levels:
            x, y = a[1][s:e], b[1][s:e]
            assert float((x - y).norm()) <= DET_VS_DEFAULT * float(x.norm()) + 1e-30, (s, e)
        if b[2] is not None and lo < hg.n_params():
            x, y = a[2], b[2]
            assert float((x - y).abs().max()) < 1e-2 * max(1.0, float(y.abs().max()))
            assert float((x - y).norm()) < 1e-3 * float(y.norm())


# --------------------------------------------------------------------------------------------------- A.5 non-finite and range
def _mlp_case(torch, api, W, L, E, n, seed, act=1):
    rng = np.random.default_rng(seed)
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E, output_activation=act)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(W, L, E, seed=seed)))
    Sp = api.padded_samples(n)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    encT[:, :n] = _dev(torch, rng.uniform(0, 1, (E, n)).astype(np.float16))
    return net, encT, rng


def _both_modes_mlp(torch, api, net, encT, dout, n, recompute):
    res = []
    for det in (False, True):
        if det:
            _shadows(api, n_mlp=net.n_params())
        dp = torch.zeros(net.n_params(), device="cuda")
        if recompute:
            out = net.train_forward_outputs(encT, n)
            net.train_backward_recompute(encT, out, dout, n, dp)
        else:
            ws = net.train_workspace(n)
            out = net.train_forward(encT, n, ws)
            net.train_backward(encT, out, dout, n, ws, dp)
        torch.cuda.synchronize()
        api.set_deterministic(None, None)
        res.append(dp.double())
    return res


@pytest.mark.parametrize("W,recompute", [(64, True), (128, False)])
def test_non_finite_gradients_stay_non_finite_in_both_modes(gpu, oracle, W, recompute):
    """An Inf in one dout entry (weight gradients) and a NaN in one denc entry (hash scatter): the set of non-finite gradient
    elements is the same in both modes -- the fixed point used to turn them into finite numbers -- and every other element
    agrees with the default mode (weight gradients: DET_VS_DEFAULT per element of the finite part's norm; scatter: the
    float64 bound of test_deterministic_hash_scatter_matches_float64)."""
    torch = gpu
    from rtx_nerf_amd import api
    n = 3000
    net, encT, rng = _mlp_case(torch, api, W, 2, 48, n, seed=W)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    dout[1234, 1] = np.inf
    a, b = _both_modes_mlp(torch, api, net, encT, _dev(torch, dout), n, recompute)
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    assert not bool(fa.all()) and torch.equal(fa, fb), (int((~fa).sum()), int((~fb).sum()), int((fa != fb).sum()))
    assert float((a[fa] - b[fa]).norm()) <= DET_VS_DEFAULT * float(a[fa].norm())
    # the scatter: NaN in one denc entry
    hg = api.HashGrid(8, 2, 14, 8, 1.6, n_dir_freqs=4)
    ocfg = oracle.hg_cfg(8, 2, 14, 8, 1.6)
    P = 300
    _, _, _, samples = _segments(torch, api, rng, P, 0)
    S = 32 * P
    E, Sp = hg.encoded_width(), api.padded_samples(S)
    denc = np.zeros((E, Sp), np.float16)
    denc[:16, :S] = (rng.standard_normal((16, S)) * 0.5).astype(np.float16)
    denc[5, 777] = np.nan
    want = oracle.hg_backward(ocfg, samples.cpu().numpy(), denc[:, :S].T.copy()).astype(np.float64)
    res = []
    for det in (False, True):
        if det:
            _shadows(api, n_table=hg.n_params())
        dt = torch.zeros(hg.n_params(), device="cuda")
        hg.backward(samples, _dev(torch, denc), dt)
        torch.cuda.synchronize()
        api.set_deterministic(None, None)
        res.append(dt.double().cpu().numpy())
    fa, fb = np.isfinite(res[0]), np.isfinite(res[1])
    assert np.array_equal(fa, fb) and not fa.all()
    assert np.all(~np.isfinite(want) <= ~fb)                            # every entry the NaN reaches in float64 is NaN here
    dabs = np.abs(denc[:, :S].T.astype(np.float64))
    dabs[~np.isfinite(dabs)] = 0
    A = oracle.hg_backward(ocfg, samples.cpu().numpy(), dabs.astype(np.float16)).astype(np.float64) * (1 + 4 * U)
    ok = fb & np.isfinite(want)
    assert np.all(np.abs(res[1][ok] - want[ok]) <= _scatter_bound(want[ok], A[ok], 8 * S))


@pytest.mark.parametrize("W,recompute", [(64, True), (128, False)])
def test_out_of_range_flush_is_nan_never_finite_and_wrong(gpu, W, recompute):
    """dout near the fp16 maximum on one output channel over one workgroup's samples: the output layer's flush for that channel
    passes 2^22 (int64 of v x 2^40 has no defined result from 2^23 on).  Every deterministic element is either within 1e-5 of the
    default mode's value or NaN -- never finite and wrong; the large elements are NaN, the rest are unchanged."""
    torch = gpu
    from rtx_nerf_amd import api
    n = 256                                         # one tile: every element takes exactly one flush, so no sum can wrap
    net, encT, rng = _mlp_case(torch, api, W, 1, 48, n, seed=W + 1, act=0)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    dout[:, 0] = 6.0e4
    a, b = _both_modes_mlp(torch, api, net, encT, _dev(torch, dout), n, recompute)
    nan = torch.isnan(b)
    big = a.abs() >= 2.0 ** 22
    assert bool(big.any()) and bool(nan[big].all()), (int(big.sum()), int(nan[big].sum()))
    close = (a - b).abs() <= 1e-5 * a.abs() + 1e-12
    assert bool((nan | close).all()), int((~(nan | close)).sum())
    assert bool(close[~big & torch.isfinite(a)].sum() > 0)


# ------------------------------------------------------------------------------------------------------------- A.6 stale shadow
def test_collected_deterministic_trainer_leaves_no_stale_shadow(gpu):
    """A deterministic Trainer stepped and then collected: the library must not keep adding into its freed shadows.  The caching
    allocator hands that memory to the next tensors of the same size (here: int64 sentinels); direct backward calls made
    afterwards must leave them untouched and compute what the default mode computes.  (Without the fix this fails on the
    sentinels; the freed block stays mapped, so it is an assertion, not a fault.)"""
    torch = gpu
    from rtx_nerf_amd import api
    tr = _small_trainer(torch, "hash", "nerf", 64, 2, deterministic=True)
    o, d, t = _batch(torch)
    tr.step(o, d, t)
    torch.cuda.synchronize()
    net, hg = tr.net, tr.hg
    sizes = [tr._det_mlp.numel(), tr._det_table.numel()]
    del tr
    gc.collect()
    sentinel = 0x5A5A5A5A5A5A5A5A
    keep = [torch.full((s,), sentinel, dtype=torch.int64, device="cuda") for s in sizes for _ in range(3)]
    rng = np.random.default_rng(8)
    n = 4000
    E, Sp = net.encoded_width(), api.padded_samples(n)
    encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    encT[:, :n] = _dev(torch, rng.uniform(-1, 1, (E, n)).astype(np.float16))
    dout = _dev(torch, (rng.standard_normal((n, 4)) * 0.05).astype(np.float16))
    x = _dev(torch, np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0, 3, (n, 2))], 1).astype(np.float32))
    denc = torch.zeros((hg.encoded_width(), Sp), dtype=torch.float16, device="cuda")
    denc[:16, :n] = _dev(torch, (rng.standard_normal((16, n)) * 0.5).astype(np.float16))

    def direct():
        ws = net.train_workspace(n)
        out = net.train_forward(encT, n, ws)
        dp = torch.zeros(net.n_params(), device="cuda")
        net.train_backward(encT, out, dout, n, ws, dp)
        dt = torch.zeros(hg.n_params(), device="cuda")
        hg.backward(x, denc, dt)
        torch.cuda.synchronize()
        return dp.double(), dt.double()

    got = direct()
    for k in keep:
        assert bool((k == sentinel).all()), f"a tensor allocated after the trainer died was written: {int((k != sentinel).sum())} elements"
    api.set_deterministic(None, None)
    ref = direct()
    for g, r in zip(got, ref):
        assert float((g - r).norm()) <= DET_VS_DEFAULT * float(r.norm()) and float(r.norm()) > 0
