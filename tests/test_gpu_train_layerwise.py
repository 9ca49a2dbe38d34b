"""The training forward (mlp_train_fwd_kernel) and the dgrad chain (mlp_bwd_kernel) layer by layer against float64, teacher-forced.

Every tensor the two kernels leave behind -- acts[l], the sign masks, out, dzL, dz[l], dencT -- is compared with a float64
restatement of the ONE stage that produced it, computed from the kernel's own stored inputs of that stage
(tests/_train_float64.py).  What is left between the two is one fp32 accumulation and one rounding to fp16, so the bound is
derived (half an fp16 ulp + the accumulation), not measured; tests/test_train_float64_reference.py shows on the CPU what it
catches.  With test_saved_activation_weight_gradients_match_float64, which starts from these dZ and activations, every tensor of
the saved-activation path is held per element.  The lean path's masks and dZ equal these bit for bit (tests/test_gpu_train.py)
and are decoded here once more from its own workspace; its weight gradients, which recompute the activations, and the fused
64-wide kernel's are held per element by tests/test_gpu_wgrad_float64.py against the tensors pinned here.

Shapes: 16 encoded features is one k-step; 176 is wider than W and ends on a ragged 48-row chunk in layer 0; 16, 48, 112 and 176
are all off multiples of 32 (the dencT row-tile edge); n = 700 is two tiles plus 188, so the last wave stops inside a column
tile.  Workspaces are pre-filled with an fp16 NaN pattern: what a kernel does not write is seen, what it must not read poisons.

Measured on the MI355X (largest err / bound per kind of stage; the share of values equal to fp16(ref)):
profiles/r13/train_layerwise_float64.txt.
"""
import numpy as np
import pytest

import _train_float64 as T
from rtx_nerf_amd import scenes

pytestmark = pytest.mark.gpu

CASES = [(128, 1, 48), (128, 2, 16), (128, 3, 176), (128, 8, 112), (64, 1, 16), (64, 2, 112), (64, 4, 176), (64, 5, 48)]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prefill(torch, ws):
    ws.view(torch.int16).fill_(T.SENTINEL)
    return ws


def _raw(torch, ws):
    return ws.view(torch.uint8).cpu().numpy()


def _case(torch, api, W, L, E, act, n, seed, dout_scale=1.0, dead=None):
    """dead: bool [n / 32], segments whose loss gradient is zero"""
    rng = np.random.default_rng(seed)
    params = scenes.xavier_params_fp16(W, L, E, seed=seed + 1)
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E, output_activation=act)
    net.set_params(_dev(torch, params))
    Sp = api.padded_samples(n)
    encT = np.zeros((E, Sp), np.float16)
    encT[:, :n] = rng.uniform(-1, 1, (E, n)).astype(np.float16)
    dout = (rng.standard_normal((n, 4)) * 0.05 * dout_scale).astype(np.float16)      # N(0, 0.05) in fp16
    if dead is not None:
        dout.reshape(-1, 32, 4)[dead] = 0
    return net, params, encT, dout, Sp


def _saved_run(torch, api, W, L, E, act, n, seed, **kw):
    """train_forward + train_backward over a pre-filled workspace, checked by T.check_saved; returns (report, Workspace)."""
    net, params, encT, dout, Sp = _case(torch, api, W, L, E, act, n, seed, **kw)
    encT_d = _dev(torch, encT)
    ws = _prefill(torch, net.train_workspace(n))
    assert ws.numel() * 2 == T.layout(W, L, Sp).bytes
    rad = torch.zeros((n, 4), device="cuda")
    out = net.train_forward(encT_d, n, ws, radiance=rad)
    dparams = torch.zeros(net.n_params(), device="cuda")
    dencT = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    net.train_backward(encT_d, out, _dev(torch, dout), n, ws, dparams, dencT)
    torch.cuda.synchronize()
    out_np = out.cpu().numpy()
    np.testing.assert_array_equal(rad.cpu().numpy(), out_np[:, :4].astype(np.float32))          # radiance == out[:, :4]
    report = T.Report()
    try:
        got = T.check_saved(report, _raw(torch, ws), params, W, L, E, bool(act), n, encT, out_np, dout, dencT.cpu().numpy())
    finally:
        report.print(f"{W}x{L} E{E} act{act} n{n}")
        print(report.summary(f"{W}x{L} E{E} act{act} n{n}"))
    assert bool(torch.isfinite(dparams).all()), "the weight-gradient kernels read something the chain did not write"
    return report, got


@pytest.mark.parametrize("n", [5, 256, 700])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("W,L,E", CASES)
def test_every_stage_of_the_saved_activation_path_matches_float64(gpu, W, L, E, act, n):
    torch = gpu
    from rtx_nerf_amd import api
    report, _ = _saved_run(torch, api, W, L, E, act, n, seed=W + 10 * L + E + n)
    assert len(report) == 2 * L + 3                 # acts and dz of every layer, out, dzL, dencT


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("W,L,E", [(128, 8, 112), (64, 4, 176)])
def test_small_gradients_keep_their_subnormals(gpu, W, L, E, act):
    """dout x 2^-6: most of dz[0] is below 2^-14.  The same bound: subnormal fp16 operands enter the matrix products with their
    value and subnormal results are stored, nowhere flushed -- a flush anywhere in the chain would show as an
    error of up to 2^-14 against a bound of about 2^-25."""
    torch = gpu
    from rtx_nerf_amd import api
    n = 700
    _, ws = _saved_run(torch, api, W, L, E, act, n, seed=W + L, dout_scale=2.0 ** -6)
    dz0 = ws.dz[0, :, :n].astype(np.float64)
    nz = np.abs(dz0[dz0 != 0])
    assert nz.size > 0.2 * dz0.size and (nz < 2.0 ** -14).mean() > 0.5, (nz.size, float((nz < 2.0 ** -14).mean()))


@pytest.mark.parametrize("W,L,E", [(128, 3, 48), (64, 2, 112)])
def test_a_dead_tile_between_two_live_tiles(gpu, W, L, E):
    """List-free run, the middle 256-sample tile without a loss gradient: live flag 0, dz / dzL keep the pre-fill, its dencT
    columns are zero (T.check_saved asserts exactly that of every tile flagged dead); the neighbours pass the bound."""
    torch = gpu
    from rtx_nerf_amd import api
    n = 700
    net, params, encT, dout, Sp = _case(torch, api, W, L, E, 1, n, seed=W + L + E)
    dout[256:512] = 0
    encT_d = _dev(torch, encT)
    ws = _prefill(torch, net.train_workspace(n))
    out = net.train_forward(encT_d, n, ws)
    dparams = torch.zeros(net.n_params(), device="cuda")
    dencT = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    net.train_backward(encT_d, out, _dev(torch, dout), n, ws, dparams, dencT)
    torch.cuda.synchronize()
    report = T.Report()
    got = T.check_saved(report, _raw(torch, ws), params, W, L, E, True, n, encT, out.cpu().numpy(), dout, dencT.cpu().numpy())
    print(report.summary(f"dead tile {W}x{L} E{E}"))
    assert got.live.tolist() == [1, 0, 1]
    assert T.is_sentinel(got.dz[:, :, 256:512]).all() and T.is_sentinel(got.dzL[:, 256:512]).all()
    assert not dencT[:, 256:512].float().abs().sum().item()
    assert bool(torch.isfinite(dparams).all())


@pytest.mark.parametrize("W,L,E", [(128, 3, 48), (64, 2, 112), (64, 4, 176)])
def test_live_list_forms(gpu, W, L, E):
    """train_forward_live + train_backward_live: 100 segments, a random 30 % listed, first and last forced, so the list
    ends inside a block of eight slots (those slots' dz / dzL are zeros).  T.check_live: listed segments' acts and masks in place and within the
    bound, the others keep the pre-fill; dz / dzL compact at slot * 32 + sample, within the bound of the restatement built from
    the compact tensors; dencT in place for the listed segments, untouched elsewhere."""
    torch = gpu
    from rtx_nerf_amd import api
    P = 100
    n = P * 32
    rng = np.random.default_rng(W + L)
    live = rng.random(P) < 0.3
    live[[0, P - 1]] = True
    net, params, encT, dout, Sp = _case(torch, api, W, L, E, 1, n, seed=W + L + E, dead=~live)
    encT_d, dout_d = _dev(torch, encT), _dev(torch, dout)
    lws = api.live_segments_workspace(P)
    api.live_segments(dout_d, P, P, lws)
    count = int(lws[0].item())
    live_list = lws[4:4 + count].cpu().numpy()
    np.testing.assert_array_equal(live_list, np.nonzero(live)[0])
    out = net.train_forward_outputs(encT_d, n)
    ws = _prefill(torch, net.train_workspace(n))
    net.train_forward_live(encT_d, n, ws, lws)
    dparams = torch.zeros(net.n_params(), device="cuda")
    dencT = torch.full((E, Sp), 7.0, dtype=torch.float16, device="cuda")
    net.train_backward_live(encT_d, out, dout_d, n, ws, lws, dparams, dencT)
    torch.cuda.synchronize()
    report = T.Report()
    try:
        T.check_live(report, _raw(torch, ws), params, W, L, E, True, n, live_list, encT, out.cpu().numpy(), dout, dencT.cpu().numpy(), 7.0)
    finally:
        print(report.summary(f"live list {W}x{L} E{E}"))
    assert len(report) == 2 * L + 2                  # no outputs in the live pass
    assert bool(torch.isfinite(dparams).all())


def test_lean_workspace(gpu):
    """8 x 128, n = 700 (encT form) and 22 segments (the form with sampler and encoder folded in), masks decoded from the lean
    workspace.  The encT form stores dz of every layer (the lean weight-gradient kernel reads dz[L-1] there); the segments form
    sets skip_last_dz: dz[L-1] keeps the pre-fill, and dz[L-2] is restated from the dz[L-1] the encT form stored for the same
    operands (same kernel, same masks and outputs bit for bit -- asserted first)."""
    torch = gpu
    from rtx_nerf_amd import api
    W, L, E, n = 128, 8, 112, 700
    net, params, encT, dout, Sp = _case(torch, api, W, L, E, 1, n, seed=41)
    encT_d, dout_d = _dev(torch, encT), _dev(torch, dout)
    wl = _prefill(torch, net.train_lean_workspace(n))
    assert wl.numel() * 2 == T.layout(W, L, Sp, lean=True).bytes
    out = net.train_forward_lean(encT_d, n, wl)
    dp = torch.zeros(net.n_params(), device="cuda")
    net.train_backward_lean(encT_d, out, dout_d, n, wl, dp)
    ws = _prefill(torch, net.train_workspace(n))
    out_s = net.train_forward(encT_d, n, ws)
    torch.cuda.synchronize()
    assert torch.equal(out, out_s) and bool(torch.isfinite(dp).all())
    report = T.Report()
    saved = T.check_saved(report, _raw(torch, ws), params, W, L, E, True, n, encT, out_s.cpu().numpy(), None, None)    # acts == masks
    lean = T.check_saved(report, _raw(torch, wl), params, W, L, E, True, n, encT, out.cpu().numpy(), dout, None, lean=True)
    np.testing.assert_array_equal(lean.words, saved.words)
    print(report.summary("lean 128x8 E112 n700"))
    assert len(report) == (L + 1) + (L + 1)
    # ---- sampler and encoder folded in: skip_last_dz ----
    P = 22
    n = P * 32
    rng = np.random.default_rng(5)
    net = api.Network(n_neurons=W, n_hidden_layers=L)
    assert net.lean_fused_supported()
    params = scenes.xavier_params_fp16(W, L, E, seed=6)
    net.set_params(_dev(torch, params))
    start = _dev(torch, rng.uniform(-1, 1, (P, 3)).astype(np.float32))
    end = _dev(torch, (start.cpu().numpy() + rng.uniform(-0.2, 0.2, (P, 3))).astype(np.float32))
    view = _dev(torch, rng.uniform(0, 3.0, (P, 2)).astype(np.float32))
    Sp = api.padded_samples(n)
    encT_d = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
    net.encode_frequency_segments(start, end, view, P, 0, encT_d)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    dout_d = _dev(torch, dout)
    wa, wb = _prefill(torch, net.train_lean_workspace(n)), _prefill(torch, net.train_lean_workspace(n))
    oa = net.train_forward_lean(encT_d, n, wa)
    ob = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
    net.train_forward_lean_segments(start, end, view, P, 0, wb, ob)
    dpa, dpb = torch.zeros(net.n_params(), device="cuda"), torch.zeros(net.n_params(), device="cuda")
    net.train_backward_lean(encT_d, oa, dout_d, n, wa, dpa)
    net.train_backward_lean_segments(start, end, view, P, 0, ob, dout_d, wb, dpb)
    torch.cuda.synchronize()
    assert torch.equal(oa, ob) and bool(torch.isfinite(dpb).all())
    encT = encT_d.cpu().numpy()
    report = T.Report()
    a = T.check_saved(report, _raw(torch, wa), params, W, L, E, True, n, encT, oa.cpu().numpy(), dout, None, lean=True)
    b = T.check_saved(report, _raw(torch, wb), params, W, L, E, True, n, encT, ob.cpu().numpy(), dout, None, lean=True,
                      dz_last=a.dz[L - 1, :, :n], skip_last_dz=True)
    np.testing.assert_array_equal(a.words, b.words)
    assert T.is_sentinel(b.dz[L - 1]).all()
    np.testing.assert_array_equal(a.dz[:L - 1].view(np.uint16), b.dz[:L - 1].view(np.uint16))
    np.testing.assert_array_equal(a.dzL.view(np.uint16), b.dzL.view(np.uint16))
    print(report.summary("lean 128x8 E112, 22 segments (encT form, then segments form)"))
    assert len(report) == (L + 1) + L
