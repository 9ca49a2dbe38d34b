"""The recomputing weight-gradient kernels against float64, element by element: mlp_bwd_fused64_kernel<L, KS0> (all 16
instantiations) and the lean path's wgrad_recompute_kernel / wgrad_recompute_all_kernel (three passes, both encoding sources).

The reference is dW_l = dZ_l X_l^T in float64 from the tensors the SAVED-activation path leaves in its workspace on the same
inputs (tests/test_gpu_train_layerwise.py holds those to float64 stage by stage); the bound is u |ref| + k u |dZ_l| |X_l|^T with
k derived from the kernels' loops (tests/_wgrad_float64.py) -- no flat tolerance; the deterministic mode adds the rounding of its
partials to the fixed point, 2^-41 per atomic, derived there too.  That reference applies only if the kernels under
test rebuild the saved values, which every test asserts first, bit for bit: the fused kernel's dencT against the saved chain's,
the lean path's masks, dz and dzL against the saved path's.  tests/test_wgrad_float64_reference.py shows on the CPU what the
bound catches.

Sizes: n = 700 is three tiles, the last one ragged -- its third wave stops inside a column tile, its fourth is empty;
n = 256 (2 CUs + 35) + 37 makes 35 blocks run three tiles of their persistent loop with a ragged last one;
n = 256 (4 CUs + 5) + 37 is past the threshold of the lean path's single launch.  Workspaces are pre-filled with an fp16 NaN pattern.

Measured on the MI355X (largest err / bound per case and the share of elements above half of it): profiles/r17/wgrad_float64.txt.
"""
from collections import namedtuple

import numpy as np
import pytest

import _train_float64 as T
import _wgrad_float64 as WG
from rtx_nerf_amd import scenes

pytestmark = pytest.mark.gpu

FILL = 7.0                      # what dencT holds before a call


@pytest.fixture(autouse=True)
def _restore_default_mode(gpu):
    yield
    from rtx_nerf_amd import api
    api.set_deterministic(None, None)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cus(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _prefill(torch, ws):
    ws.view(torch.int16).fill_(T.SENTINEL)
    return ws


def _bits(torch, t):
    return t.contiguous().view(torch.int16)


Views = namedtuple("Views", "acts dz dzL masks live")


def _views(torch, ws, W, L, Sp, lean=False):
    """The workspace's tensors as views on the device (the byte offsets of tests/_train_float64.py)"""
    lay = WG.layout(W, L, Sp, lean)
    assert ws.numel() * 2 == lay.bytes
    acts = None if lean else ws[lay.acts // 2:lay.dz // 2].view(L, W, Sp)
    return Views(acts, ws[lay.dz // 2:lay.dzL // 2].view(L, W, Sp), ws[lay.dzL // 2:lay.masks // 2].view(16, Sp),
                 ws[lay.masks // 2:lay.live // 2].view(torch.int16), ws.view(torch.uint8)[lay.live:lay.live + Sp // 256])


def _set_mode(api, net, det):
    if det:
        shadow = api.deterministic_shadow(net.n_params())
        api.set_deterministic(shadow, None)
        return shadow
    api.set_deterministic(None, None)
    return None


def _saved(torch, api, net, W, L, encT_d, out, dout_d, n, want_live=None, with_dencT=True):
    """The saved-activation path on the same inputs (its own forward fills acts and masks; its backward consumes the SAME out and
    dout as the path under test) and the float64 reference from its workspace, built on the device.  A tile the chain flagged
    dead holds no dZ (the pre-fill): it adds nothing, and its columns stay out of the products.
    Returns (ref, mag, dencT, Views of the workspace, the outputs the backward consumed)."""
    api.set_deterministic(None, None)
    E, Sp = encT_d.shape
    ws = _prefill(torch, net.train_workspace(n))
    out_s = net.train_forward(encT_d, n, ws)
    if out is None:
        out = out_s
    dencT = torch.full((E, Sp), FILL, dtype=torch.float16, device="cuda") if with_dencT else None
    net.train_backward(encT_d, out, dout_d, n, ws, torch.zeros(net.n_params(), device="cuda"), dencT)
    torch.cuda.synchronize()
    v = _views(torch, ws, W, L, Sp)
    live = v.live.cpu().numpy()
    if want_live is None:
        want_live = np.ones(Sp // 256, np.uint8)
    np.testing.assert_array_equal(live, np.asarray(want_live, np.uint8))
    if live.all():
        sel = slice(0, n)
    else:
        sel = torch.nonzero(v.live.bool().repeat_interleave(256)[:n]).reshape(-1)
    X = [encT_d[:, sel]] + [v.acts[l][:, sel] for l in range(L)]
    dZ = [v.dz[l][:, sel] for l in range(L)] + [v.dzL[:, sel]]
    ref, mag = WG.reference(dZ, X)
    ref, mag = ref.cpu().numpy(), mag.cpu().numpy()
    assert np.isfinite(ref).all() and np.isfinite(mag).all() and np.abs(ref).max() > 0, "the reference read something the saved path did not write"
    return ref, mag, dencT, v, out


def _assert_inside(title, dp, ref, mag, k, sizes, W, **kw):
    res = WG.check(dp.cpu().numpy(), ref, mag, k, sizes, **kw)
    print(WG.lines(title, res))
    assert res.bad == 0 and max(res.worst) <= 1, (title, res.bad, res.first, res.worst)
    assert not dp[-16 * W:].view(16, W)[4:].any(), f"{title}: rows 4..15 of the output layer"
    return res


def _inputs(torch, api, W, L, E, act, n, seed):
    rng = np.random.default_rng(seed)
    net = api.Network(n_neurons=W, n_hidden_layers=L, n_encoded_features=E, output_activation=act)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(W, L, E, seed=seed + 1)))
    Sp = api.padded_samples(n)
    encT = np.zeros((E, Sp), np.float16)                   # the padding columns stay zero (include/rtxn.h)
    encT[:, :n] = rng.uniform(-1, 1, (E, n)).astype(np.float16)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    return net, _dev(torch, encT), dout, Sp, rng


def _listed(rng, P, count=None):
    """bool [P]: about 30 % listed with the first and the last forced, or exactly `count` segments"""
    if count is None:
        live = rng.random(P) < 0.3
        live[[0, P - 1]] = True
        return live
    live = np.zeros(P, bool)
    live[rng.choice(P, count, replace=False)] = True
    return live


def _live_ws(torch, api, dout_zeroed_d, P, live):
    lws = api.live_segments_workspace(P)
    api.live_segments(dout_zeroed_d, P, P, lws)
    count = int(lws[0].item())
    np.testing.assert_array_equal(lws[4:4 + count].cpu().numpy(), np.nonzero(live)[0])
    return lws, count


# ===================================================================================================== the fused kernel
def _fused(torch, api, L, E, act, n, seed, dead_tile=None):
    """train_forward_outputs + train_backward_recompute in both modes against the saved path's tensors.  dead_tile: a 256-sample
    tile without a loss gradient (no list): its dencT columns are zero, the gradient is inside the same bound."""
    W = 64
    net, encT_d, dout, Sp, _ = _inputs(torch, api, W, L, E, act, n, seed)
    assert net.recompute_supported()
    want_live = np.ones(Sp // 256, np.uint8)
    if dead_tile is not None:
        dout[256 * dead_tile:256 * (dead_tile + 1)] = 0
        want_live[dead_tile] = 0
    dout_d = _dev(torch, dout)
    out = net.train_forward_outputs(encT_d, n)
    ref, mag, de_ref, _, _ = _saved(torch, api, net, W, L, encT_d, out, dout_d, n, want_live)
    tiles = WG.n_tiles_of(n)
    grid = WG.persistent_grid(tiles, _cus(torch))
    k = WG.k_recompute(tiles, grid)
    sizes = WG.layer_sizes(W, L, E)
    got = {}
    for det in (False, True):
        shadow = _set_mode(api, net, det)
        dp = torch.zeros(net.n_params(), device="cuda")
        de = torch.full((E, Sp), FILL, dtype=torch.float16, device="cuda")
        net.train_backward_recompute(encT_d, out, dout_d, n, dp, de)
        torch.cuda.synchronize()
        # the precondition of the reference: the recomputed chain is the saved one
        assert torch.equal(_bits(torch, de), _bits(torch, de_ref)), "dencT differs from the saved chain's: the reference does not apply"
        if dead_tile is not None:
            assert not de[:, 256 * dead_tile:256 * (dead_tile + 1)].any()
        _assert_inside(f"fused 64x{L} E{E} act{act} n{n}{'' if dead_tile is None else f' dead tile {dead_tile}'} det={int(det)}", dp, ref, mag, k, sizes, W,
                       det_atomics=grid if det else None)
        if det:
            assert int(shadow.abs().max()) == 0
        got[det] = dp
    api.set_deterministic(None, None)
    return net, encT_d, out, dout_d, got, (ref, mag, k, grid, sizes)


@pytest.mark.parametrize("E", [16, 32, 48, 64])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_fused_every_instantiation_three_tiles_ragged(gpu, L, E):
    from rtx_nerf_amd import api
    _fused(gpu, api, L, E, 1, 700, seed=100 * L + E)


@pytest.mark.parametrize("L,E", [(1, 32), (2, 16), (3, 64), (4, 48)])
def test_fused_without_output_activation(gpu, L, E):
    from rtx_nerf_amd import api
    _fused(gpu, api, L, E, 0, 700, seed=100 * L + E + 1)


@pytest.mark.parametrize("n", [5, 256])
@pytest.mark.parametrize("L,E", [(1, 16), (2, 48), (4, 64)])
def test_fused_one_tile(gpu, L, E, n):
    from rtx_nerf_amd import api
    _fused(gpu, api, L, E, 1, n, seed=100 * L + E + n)


@pytest.mark.parametrize("L,E", [(1, 16), (4, 64)])
def test_fused_three_tiles_deep_in_the_persistent_loop(gpu, L, E):
    """256 (2 CUs + 35) + 37 samples: every block runs two tiles, 35 of them a third, and the last tile is ragged"""
    from rtx_nerf_amd import api
    _fused(gpu, api, L, E, 1, 256 * (2 * _cus(gpu) + 35) + 37, seed=L + E)


@pytest.mark.parametrize("dead_tile", [0, 3, 5])
def test_fused_dead_tile_without_a_list(gpu, dead_tile):
    from rtx_nerf_amd import api
    _fused(gpu, api, 2, 48, 1, 1536, seed=40 + dead_tile, dead_tile=dead_tile)


@pytest.mark.parametrize("count", [None, 1, 8, 9])
def test_fused_live_form(gpu, count):
    """100 segments, about 30 % listed with the first and the last forced (the list ends inside a block of eight slots), and lists
    of exactly 1, 8 and 9.  The kernel under test gets a loss gradient on EVERY segment and must visit the listed ones only: the
    reference is the saved path run list-free with dout zeroed on the others.  Listed dencT columns equal the saved chain's bit
    for bit, the others keep what they held."""
    torch = gpu
    from rtx_nerf_amd import api
    W, L, E, P = 64, 3, 48, 100
    n = 32 * P
    net, encT_d, dout, Sp, rng = _inputs(torch, api, W, L, E, 1, n, seed=60 + (count or 0))
    live = _listed(rng, P, count)
    zeroed = dout.copy()
    zeroed.reshape(P, 32, 4)[~live] = 0
    lws, listed = _live_ws(torch, api, _dev(torch, zeroed), P, live)
    out = net.train_forward_outputs(encT_d, n)
    tile_live = np.zeros(Sp // 256, np.uint8)
    tile_live[:-(-P // 8)] = np.pad(live, (0, -P % 8)).reshape(-1, 8).any(1)
    ref, mag, de_ref, _, _ = _saved(torch, api, net, W, L, encT_d, out, _dev(torch, zeroed), n, tile_live)
    tiles = WG.n_tiles_of(n, listed=listed)
    grid = WG.persistent_grid(tiles, _cus(torch))
    col_listed = _dev(torch, np.pad(np.repeat(live, 32), (0, Sp - n)))
    dout_d = _dev(torch, dout)
    for det in (False, True):
        _set_mode(api, net, det)
        dp = torch.zeros(net.n_params(), device="cuda")
        de = torch.full((E, Sp), FILL, dtype=torch.float16, device="cuda")
        net.train_backward_recompute_live(encT_d, out, dout_d, n, lws, dp, de)
        torch.cuda.synchronize()
        assert torch.equal(_bits(torch, de[:, col_listed]), _bits(torch, de_ref[:, col_listed])), "listed dencT columns differ from the saved chain's"
        assert bool((de[:, ~col_listed] == FILL).all()), "an unlisted dencT column was written"
        _assert_inside(f"fused live 64x{L} E{E} listed {listed} of {P} det={int(det)}", dp, ref, mag, WG.k_recompute(tiles, grid),
                       WG.layer_sizes(W, L, E), W, det_atomics=grid if det else None)


def test_fused_without_dencT_is_the_same_gradient(gpu):
    """Deterministic mode, dencT = NULL (models whose encoding has no parameters): dparams bit-identical to the run with dencT"""
    torch = gpu
    from rtx_nerf_amd import api
    net, encT_d, out, dout_d, got, _ = _fused(torch, api, 3, 32, 1, 700, seed=77)
    _set_mode(api, net, True)
    dp = torch.zeros(net.n_params(), device="cuda")
    net.train_backward_recompute(encT_d, out, dout_d, 700, dp, None)
    torch.cuda.synchronize()
    assert torch.equal(dp, got[True])


def test_fused_accumulates_into_what_dparams_holds(gpu):
    torch = gpu
    from rtx_nerf_amd import api
    W, L, E, n = 64, 2, 48, 700
    net, encT_d, out, dout_d, got, (ref, mag, k, grid, sizes) = _fused(torch, api, L, E, 1, n, seed=88)
    pre = _dev(torch, np.random.default_rng(1).standard_normal(net.n_params()).astype(np.float32))
    for det in (False, True):
        _set_mode(api, net, det)
        dp = pre.clone()
        net.train_backward_recompute(encT_d, out, dout_d, n, dp, None)
        torch.cuda.synchronize()
        if det:
            assert torch.equal(dp, pre + got[True]), "deterministic: pre + (the run into zeros), bit for bit"
        else:
            res = WG.check(dp.cpu().numpy(), ref, mag, k, sizes, pre=pre.cpu().numpy(), grid=grid)
            print(WG.lines("fused accumulate 64x2 E48 n700 det=0", res))
            assert res.bad == 0 and max(res.worst) <= 1, (res.bad, res.worst)


# ===================================================================================================== the lean path
LW, LL, LE = 128, 8, 112


def _lean_net(torch, api, seed):
    net = api.Network(n_neurons=LW, n_hidden_layers=LL)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(LW, LL, LE, seed=seed)))
    assert net.lean_supported() and net.lean_fused_supported()
    return net


def _segments(torch, rng, P):
    start = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    end = (start + rng.uniform(-0.2, 0.2, (P, 3))).astype(np.float32)
    view = rng.uniform(0, 3.0, (P, 2)).astype(np.float32)
    return _dev(torch, start), _dev(torch, end), _dev(torch, view)


def _lean(torch, api, form, n, seed, live=None, dead_segments=None, single_launch=False, pre=None):
    """form "encT": train_forward_lean + train_backward_lean over n samples of a random encoding; "segments": the pair with the
    encoder folded in over n / 32 segments, the reference built from the staged encT of the same segments.  live: bool per segment
    -- the path under test walks the list with a loss gradient on every segment, the reference runs list-free with dout zeroed on
    the unlisted ones.  Both modes.  Returns the default-mode result of the last run for the accumulate test."""
    W, L, E = LW, LL, LE
    rng = np.random.default_rng(seed)
    net = _lean_net(torch, api, seed + 1)
    Sp = api.padded_samples(n)
    seg = None
    if form == "segments" or live is not None:
        assert n % 32 == 0
    if form == "segments":
        P = n // 32
        seg = _segments(torch, rng, P)
        encT_d = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
        net.encode_frequency_segments(*seg, P, 0, encT_d)
    else:
        encT = np.zeros((E, Sp), np.float16)
        encT[:, :n] = rng.uniform(-1, 1, (E, n)).astype(np.float16)
        encT_d = _dev(torch, encT)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    want_live = np.ones(Sp // 256, np.uint8)
    zeroed = dout
    lws = listed = None
    if dead_segments is not None:
        dout.reshape(-1, 32, 4)[dead_segments] = 0
        assert dead_segments.start % 8 == 0 and dead_segments.stop % 8 == 0
        want_live[dead_segments.start // 8:dead_segments.stop // 8] = 0
    if live is not None:
        P = n // 32
        zeroed = dout.copy()
        zeroed.reshape(P, 32, 4)[~live] = 0
        lws, listed = _live_ws(torch, api, _dev(torch, zeroed), P, live)
        want_live[:-(-P // 8)] = np.pad(live, (0, -P % 8)).reshape(-1, 8).any(1)
    dout_d = _dev(torch, dout)
    ref, mag, _, sv, out_s = _saved(torch, api, net, W, L, encT_d, None, _dev(torch, zeroed), n, want_live, with_dencT=False)
    n_cu = _cus(torch)
    tiles = WG.n_tiles_of(n, listed=listed)
    assert WG.all_pass_used(tiles, n_cu, form == "segments") == single_launch, "the size does not select the kernel this case is about"
    grid = WG.all_pass_grid(n_cu, form == "segments") if single_launch else WG.persistent_grid(tiles, n_cu)
    k = WG.k_recompute(tiles, grid)
    sizes = WG.layer_sizes(W, L, E)
    atomics = WG.lean_atomics(8 * (n_cu // 8) if single_launch else grid, L)     # deterministic mode: partials per element and layer
    stored = L - 1 if form == "segments" else L                # the folded form leaves dz[L-1] to its weight-gradient kernel
    if live is not None:
        lst = np.nonzero(live)[0]
        src = _dev(torch, T.compact_columns(lst))              # where the list-free chain put the listed segments' dZ
        dst = slice(0, 32 * lst.size)                          # ... and where the chain with a list puts it
    last = None
    for det in (False, True):
        _set_mode(api, net, det)
        wl = _prefill(torch, net.train_lean_workspace(n))
        out = torch.zeros((n, 16), dtype=torch.float16, device="cuda")
        dp = torch.zeros(net.n_params(), device="cuda") if pre is None else pre.clone()
        if form == "segments":
            net.train_forward_lean_segments(*seg, n // 32, 0, wl, out)
            net.train_backward_lean_segments(*seg, n // 32, 0, out, dout_d, wl, dp, live_ws=lws)
        else:
            net.train_forward_lean(encT_d, n, wl, out)
            net.train_backward_lean(encT_d, out, dout_d, n, wl, dp, live_ws=lws)
        torch.cuda.synchronize()
        # ---- the precondition: same outputs, masks, dZ ----
        lv = _views(torch, wl, W, L, Sp, lean=True)
        assert torch.equal(_bits(torch, out), _bits(torch, out_s)), "outputs differ from the saving forward's"
        assert torch.equal(lv.masks, sv.masks), "masks differ from the saving forward's"
        if live is None:
            assert torch.equal(lv.live, sv.live)
            assert torch.equal(_bits(torch, lv.dz[:stored]), _bits(torch, sv.dz[:stored])), "dz differs from the saved chain's"
            assert torch.equal(_bits(torch, lv.dzL), _bits(torch, sv.dzL)), "dzL differs from the saved chain's"
        else:
            assert torch.equal(_bits(torch, lv.dz[:stored, :, dst]), _bits(torch, sv.dz[:stored][:, :, src])), "compact dz differs from the saved chain's"
            assert torch.equal(_bits(torch, lv.dzL[:, dst]), _bits(torch, sv.dzL[:, src])), "compact dzL differs from the saved chain's"
        if stored < L:
            assert bool((_bits(torch, lv.dz[L - 1]) == T.SENTINEL).all()), "the folded form stores no dz[L-1]"
        title = (f"lean {form} n{n}" + (f" listed {listed}" if live is not None else "") + (" dead tiles" if dead_segments is not None else "")
                 + (" single launch" if single_launch else "") + f" det={int(det)}")
        if pre is None:
            _assert_inside(title, dp, ref, mag, k, sizes, W, det_atomics=atomics if det else None)
        elif det:
            last_det = torch.zeros(net.n_params(), device="cuda")
            if form == "segments":
                net.train_backward_lean_segments(*seg, n // 32, 0, out, dout_d, wl, last_det, live_ws=lws)
            else:
                net.train_backward_lean(encT_d, out, dout_d, n, wl, last_det, live_ws=lws)
            torch.cuda.synchronize()
            assert torch.equal(dp, pre + last_det), "deterministic: pre + (the run into zeros), bit for bit"
        else:
            res = WG.check(dp.cpu().numpy(), ref, mag, k, sizes, pre=pre.cpu().numpy(), grid=WG.lean_atomics(grid, L))
            print(WG.lines(title + " accumulate", res))
            assert res.bad == 0 and max(res.worst) <= 1, (res.bad, res.worst)
        last = dp
    api.set_deterministic(None, None)
    return last


@pytest.mark.parametrize("n", [5, 700])
def test_lean_encT_form(gpu, n):
    from rtx_nerf_amd import api
    _lean(gpu, api, "encT", n, seed=n)


def test_lean_segments_form_with_the_encoder_folded_in(gpu):
    from rtx_nerf_amd import api
    _lean(gpu, api, "segments", 32 * 22, seed=22)


@pytest.mark.parametrize("form", ["encT", "segments"])
def test_lean_live_form(gpu, form):
    from rtx_nerf_amd import api
    P = 100
    _lean(gpu, api, form, 32 * P, seed=31, live=_listed(np.random.default_rng(32), P))


def test_lean_list_free_with_four_dead_tiles(gpu):
    from rtx_nerf_amd import api
    _lean(gpu, api, "encT", 32 * 100, seed=33, dead_segments=slice(8, 40))


@pytest.mark.parametrize("form", ["encT", "segments"])
def test_lean_per_pass_kernels_three_tiles_deep(gpu, form):
    from rtx_nerf_amd import api
    n = 256 * (2 * _cus(gpu) + 35) + 37
    _lean(gpu, api, form, n if form == "encT" else -(-n // 32) * 32, seed=34)


@pytest.mark.parametrize("form", ["encT", "segments"])
def test_lean_single_launch(gpu, form):
    from rtx_nerf_amd import api
    n = 256 * (4 * _cus(gpu) + 5) + 37
    _lean(gpu, api, form, n if form == "encT" else -(-n // 32) * 32, seed=35, single_launch=True)


def test_lean_accumulates_into_what_dparams_holds(gpu):
    torch = gpu
    from rtx_nerf_amd import api
    n_params = LW * LE + (LL - 1) * LW * LW + 16 * LW
    pre = _dev(torch, np.random.default_rng(2).standard_normal(n_params).astype(np.float32))
    _lean(torch, api, "encT", 700, seed=36, pre=pre)
