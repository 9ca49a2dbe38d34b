"""Every ring phase of the persistent inference kernels, bit for bit.

mlp_fwd16_kernel (64 / 128 wide) and mlp_fwd256x16_kernel loop over tiles and carry the state of a three-slot LDS weight
ring from one tile to the next: `qs % 3` with the wrap-around prefetch (`lk >= n_layers`, `exists = more`) and the one-stage
skew between the two wave groups in the first, `gq % 3` over 4 * n_hidden + 1 chunks per tile in the second.  Which slot a
tile starts on depends on (n_hidden - 1) mod 3 resp. (4 * n_hidden + 1) mod 3 and on how many tiles the block has done, so
a stale-slot or lost-wait defect can sit at ONE depth and ONE tile ordinal.  The property tested is exact: a sample's
output does not depend on where in the batch it sits.  A launch large enough that blocks take 2, 3 and 4 tiles is filled
with repetitions of a small base set; every copy must equal the base set's output from a launch of its own, in which no
block runs a second tile.

Sizing: the grid is G = CUs - 64 blocks (rtxn_mlp_set_reserved_cus(64): the smallest grid the ABI allows, and that entry
point's test).  n_tiles = 2G + G/2 (blocks take 2 or 3 tiles) and 3G + G/2 (3 or 4): a block's last tile is its 2nd, 3rd and
4th, i.e. on each of the three ring phases whatever the depth.  Both launches end one segment / 37 samples past a tile
boundary.  Base set: 1,237 samples (1,237 mod 16, 64, 512 = 5, 21, 213: copies land on every column, wave and tile offset)
resp. 77 segments (odd: a segment alternates between the two slots of a wave).  Repetition and comparison run on the device.

The hash kernels (hashmlp_fwd_kernel, mlp_enc_fwd16_kernel) hold all weights in LDS and have no ring, but each wave reuses
its registers and (the fused one) its LDS transposition strip from tile to tile: same construction, every wave >= 3 tiles.
"""
import numpy as np
import pytest

import _mlp_float64 as F64

pytestmark = pytest.mark.gpu

RESERVED = 64
N_BASE, SEG_BASE = F64.N_BASE, 77
DEPTHS = list(range(1, 9))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grid(torch, reserved=RESERVED):
    g = torch.cuda.get_device_properties(0).multi_processor_count - reserved
    assert g >= 2
    return g


def _tile(W):
    return 256 if W == 256 else 512                      # samples per block per iteration; segments: / 32


def _tile_counts(G):
    return [2 * G + G // 2, 3 * G + G // 2]


def _repeat_to(t, n):
    """The first n rows of t repeated end to end (on the device)."""
    reps = (n + t.shape[0] - 1) // t.shape[0]
    return t.repeat(reps, *([1] * (t.dim() - 1)))[:n].contiguous()


def _assert_copies(torch, big, base, n, sentinel, what, rows_per_tile, G):
    """big[:n] is base repeated end to end, bit for bit; big[n:] still holds the sentinel."""
    nb = base.shape[0]
    k, rem = divmod(n, nb)
    ok = torch.equal(big[:k * nb].reshape(k, nb, -1), base.reshape(1, nb, -1).expand(k, nb, -1)) and \
        torch.equal(big[k * nb:n], base[:rem])
    if not ok:                                            # say WHERE: tile numbers, and which of the block's tiles they are
        bad = (big[:n].reshape(n, -1) != _repeat_to(base, n).reshape(n, -1)).any(dim=1).nonzero().flatten()
        tiles = torch.unique(bad // rows_per_tile).cpu().numpy()
        ordinals = sorted(set((tiles // G).tolist()))
        raise AssertionError(f"{what}: {bad.numel()} of {n} rows differ from the single-tile launch, in {tiles.size} tiles "
                             f"(first {tiles[:8].tolist()}), tile ordinals within their blocks {ordinals}")
    assert bool((big[n:] == sentinel).all()), f"{what}: rows past the live count were written"


@pytest.fixture(scope="module")
def base(gpu):
    """The base sets, on the device, shared and never modified: samples, segments, and their repetitions by length."""
    torch = gpu
    x = F64.base_inputs(N_BASE, seed=0)
    rng = np.random.default_rng(77)
    start = rng.uniform(-1, 1, (SEG_BASE, 3)).astype(np.float32)
    end = rng.uniform(-1, 1, (SEG_BASE, 3)).astype(np.float32)
    view = np.stack([rng.uniform(0, 3.1416, SEG_BASE), rng.uniform(-3.1416, 3.1416, SEG_BASE)], axis=1).astype(np.float32)
    b = dict(x=_dev(torch, x), start=_dev(torch, start), end=_dev(torch, end), view=_dev(torch, view), big={})

    def big(name, n):
        if (name, n) not in b["big"]:
            b["big"][(name, n)] = _repeat_to(b[name], n)
        return b["big"][(name, n)]
    b["repeat"] = big
    return b


def _net(torch, api, W, ndf, depth, act, reserved=RESERVED, gain=1):
    net = api.Network(n_neurons=W, n_hidden_layers=depth, n_dir_freqs=ndf, output_activation=act)
    net.set_params(_dev(torch, F64.gained_params(W, depth, net.encoded_width(), seed=7 * W + depth + ndf, gain=gain)))
    net.set_reserved_cus(reserved)
    return net


def _run_samples(torch, net, x, pad=64):
    n = x.shape[0]
    out = torch.full((n + pad, 16), -5.0, dtype=torch.float16, device="cuda")
    rad = torch.full((n + pad, 4), -5.0, device="cuda")
    net.forward(x, out[:n])
    net.forward_radiance(x, rad[:n])
    return out, rad


def _run_segments(torch, net, start, end, view, live, cap):
    """start / end / view hold `cap` rows, `live` of them count."""
    total = torch.tensor([live], dtype=torch.int32, device="cuda")
    rad = torch.full((cap * 32, 4), -3.0, device="cuda")
    tv = torch.full((cap * 32,), -3.0, device="cuda")
    half = torch.full((cap * 32, 4), -3.0, dtype=torch.float16, device="cuda")
    net.forward_segments(start, end, view, total, cap, rad, tv)
    net.forward_segments_compact(start, end, view, total, cap, half)
    return rad, tv, half


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("W,ndf", F64.VARIANTS)
def test_output_does_not_depend_on_the_tile(gpu, base, W, ndf, depth):
    torch = gpu
    from rtx_nerf_amd import api
    G, tile = _grid(torch), _tile(W)
    tsegs = tile // 32
    net = _net(torch, api, W, ndf, depth, api.ACT_NONE)     # linear output: every bit of the logits is compared
    pad = 13
    # ---- the base launches: no block runs a second tile
    assert (N_BASE + tile - 1) // tile <= G and (SEG_BASE + tsegs - 1) // tsegs <= G
    out0, rad0 = _run_samples(torch, net, base["x"])
    seg_in = [base["repeat"](k, SEG_BASE + pad) for k in ("start", "end", "view")]
    srad0, stv0, shalf0 = _run_segments(torch, net, *seg_in, SEG_BASE, SEG_BASE + pad)
    torch.cuda.synchronize()
    S0 = SEG_BASE * 32
    assert bool((out0[N_BASE:] == -5.0).all()) and bool((rad0[N_BASE:] == -5.0).all())
    assert bool((srad0[S0:] == -3.0).all()) and bool((stv0[S0:] == -3.0).all()) and bool((shalf0[S0:] == -3.0).all())
    out0, rad0, srad0, stv0, shalf0 = out0[:N_BASE], rad0[:N_BASE], srad0[:S0], stv0[:S0], shalf0[:S0]
    assert bool(torch.isfinite(out0.float()).all()) and float(out0.float().std()) > 1e-3
    # the four entry points agree with each other, bit for bit, at this depth
    assert torch.equal(rad0, out0[:, :4].float()), "forward_radiance != columns 0..3 of forward"
    samples = torch.zeros((S0, 5), device="cuda")
    t_ref = torch.zeros((S0,), device="cuda")
    ones = torch.ones(SEG_BASE, dtype=torch.int32, device="cuda")
    idx = torch.arange(SEG_BASE, dtype=torch.int32, device="cuda")
    api.launchSampler(base["start"], base["end"], base["view"], t_ref, samples, SEG_BASE, 8, ones, idx, api.SAMPLING_REGULAR)
    assert torch.equal(srad0, net.forward_radiance(samples)), "forward_segments != forward_radiance on the sampler's samples"
    assert torch.equal(stv0, t_ref), "forward_segments' t_vals != the sampler's"
    assert torch.equal(shalf0, srad0.to(torch.float16)) and torch.equal(shalf0.float(), srad0), "compact != fp16 of float4"
    # ---- total_segments = 0 with capacity: nothing is written
    nrad, ntv, nhalf = _run_segments(torch, net, *seg_in, 0, SEG_BASE + pad)
    assert bool((nrad == -3.0).all()) and bool((ntv == -3.0).all()) and bool((nhalf == -3.0).all())
    # ---- the multi-tile launches
    for n_tiles in _tile_counts(G):
        assert 2 * G < n_tiles < 4 * G
        n = (n_tiles - 1) * tile + 37
        out, rad = _run_samples(torch, net, base["repeat"]("x", n))
        tag = f"{depth} x {W} ({ndf} octaves), {n_tiles} tiles on {G} blocks"
        _assert_copies(torch, out, out0, n, -5.0, "forward, " + tag, tile, G)
        _assert_copies(torch, rad, rad0, n, -5.0, "forward_radiance, " + tag, tile, G)
        live = (n_tiles - 1) * tsegs + 1
        cap = live + pad
        srad, stv, shalf = _run_segments(torch, net, *[base["repeat"](k, cap) for k in ("start", "end", "view")], live, cap)
        _assert_copies(torch, srad, srad0, live * 32, -3.0, "forward_segments, " + tag, tile, G)
        _assert_copies(torch, stv, stv0, live * 32, -3.0, "forward_segments t_vals, " + tag, tile, G)
        _assert_copies(torch, shalf, shalf0, live * 32, -3.0, "forward_segments_compact, " + tag, tile, G)


@pytest.mark.parametrize("W,ndf", F64.VARIANTS)
def test_reserved_cus_change_the_grid_not_the_bits(gpu, base, W, ndf):
    """rtxn_mlp_set_reserved_cus: 0 and 64 reserved CUs (blocks take 2..3 resp. 3..4 tiles of the same launch) give identical
    bits through all four entry points -- with the sigmoid, the shipped configuration; the range check holds."""
    torch = gpu
    from rtx_nerf_amd import api, _lib
    G, tile = _grid(torch), _tile(W)
    depth = 5
    n_tiles = _tile_counts(G)[1]
    n, live = (n_tiles - 1) * tile + 37, (n_tiles - 1) * (tile // 32) + 1
    cap = live + 13
    got = []
    for reserved in (0, RESERVED):
        net = _net(torch, api, W, ndf, depth, api.ACT_SIGMOID, reserved=reserved, gain=2)
        got.append(_run_samples(torch, net, base["repeat"]("x", n)) +
                   _run_segments(torch, net, *[base["repeat"](k, cap) for k in ("start", "end", "view")], live, cap))
    for a, b, name in zip(got[0], got[1], ("forward", "forward_radiance", "forward_segments", "t_vals", "compact")):
        assert torch.equal(a, b), f"{name}: {W} wide, {ndf} octaves"
    o = got[0][0][:n].float()
    assert bool(((o >= 0) & (o <= 1)).all()) and float(o.std()) > 0.01
    for bad in (-1, 65):
        with pytest.raises(_lib.RtxnError, match="out of"):
            net.set_reserved_cus(bad)


# ---------------------------------------------------------------------------------------------------- the hash path
HASH_DEPTHS = [1, 2, 3, 4, 8]
PER_CU = 3                                               # upper bound of the occupancy-derived blocks per CU (persistent_grid)


@pytest.mark.parametrize("depth", HASH_DEPTHS)
def test_hash_output_does_not_depend_on_the_wave_tile(gpu, base, depth):
    """rtxn_hashmlp_forward_segments: a wave tile is 2 segments, a block 4 waves, the grid at most 3 blocks per CU.  3.5 x 4 x 3
    x G wave tiles (about 16,000 segments): every wave takes at least 3 tiles whatever the occupancy."""
    torch = gpu
    from rtx_nerf_amd import api
    G = _grid(torch)
    hg = api.HashGrid(4, 2, 10, 8, 1.6, n_dir_freqs=4)
    E = hg.encoded_width()
    net = api.Network(n_neurons=64, n_hidden_layers=depth, n_encoded_features=E, output_activation=api.ACT_NONE)
    assert api.hashmlp_supported(net, hg)
    net.set_params(_dev(torch, F64.gained_params(64, depth, E, seed=depth)))
    net.set_reserved_cus(RESERVED)
    table = _dev(torch, np.random.default_rng(depth).uniform(-0.5, 0.5, hg.n_params()).astype(np.float16))
    stype = api.SAMPLING_MIDPOINT_WORLD if depth % 2 == 0 else api.SAMPLING_REGULAR

    def run(live, cap):
        seg_in = [base["repeat"](k, cap) for k in ("start", "end", "view")]
        total = torch.tensor([live], dtype=torch.int32, device="cuda")
        rad = torch.full((cap * 32, 4), -3.0, dtype=torch.float16, device="cuda")
        step = torch.full((cap,), -3.0, device="cuda")
        api.hashmlp_forward_segments(net, hg, table, *seg_in, total, cap, rad, stype, 7.5, step)
        return rad, step

    assert (SEG_BASE + 1) // 2 <= 4 * G
    rad0, step0 = run(SEG_BASE, SEG_BASE + 37)
    torch.cuda.synchronize()
    assert bool((rad0[SEG_BASE * 32:] == -3.0).all()) and bool((step0[SEG_BASE:] == -3.0).all())
    rad0, step0 = rad0[:SEG_BASE * 32], step0[:SEG_BASE]
    assert bool(torch.isfinite(rad0.float()).all()) and float(rad0.float().std()) > 1e-3
    live = 2 * (7 * 4 * PER_CU * G // 2) + 1                 # odd: the last wave tile is half empty
    assert (live + 1) // 2 >= 3 * 4 * PER_CU * G
    rad, step = run(live, live + 37)
    tag = f"hashmlp_forward_segments, {depth} x 64, {live} segments"
    _assert_copies(torch, rad, rad0, live * 32, -3.0, tag, 64, 4 * PER_CU * G)
    if stype == api.SAMPLING_MIDPOINT_WORLD:
        _assert_copies(torch, step, step0, live, -3.0, tag + " (segment_step)", 2, 4 * PER_CU * G)
    else:
        assert bool((step == -3.0).all())                    # REGULAR: no step is written
    nrad, nstep = run(0, SEG_BASE)
    assert bool((nrad == -3.0).all()) and bool((nstep == -3.0).all())


@pytest.mark.parametrize("E", [32, 64])
@pytest.mark.parametrize("depth", HASH_DEPTHS)
def test_pre_encoded_output_does_not_depend_on_the_wave_tile(gpu, depth, E):
    """rtxn_mlp_train_forward_outputs (mlp_enc_fwd16_kernel; its grid ignores the reservation): 3.5 x 4 x 3 x CUs wave tiles of 64
    samples, so every wave takes at least 3."""
    torch = gpu
    from rtx_nerf_amd import api
    cus = _grid(torch, 0)
    net = api.Network(n_neurons=64, n_hidden_layers=depth, n_encoded_features=E, output_activation=api.ACT_NONE)
    net.set_params(_dev(torch, F64.gained_params(64, depth, E, seed=depth + E)))
    feat = _dev(torch, np.random.default_rng(E + depth).uniform(-1, 1, (E, N_BASE)).astype(np.float16))

    def run(S):
        Sp = api.padded_samples(S)
        encT = torch.zeros((E, Sp), dtype=torch.float16, device="cuda")
        reps = (S + N_BASE - 1) // N_BASE
        encT[:, :S] = feat.repeat(1, reps)[:, :S]
        out = torch.full((S + 64, 16), -5.0, dtype=torch.float16, device="cuda")
        rad = torch.full((S + 64, 4), -5.0, device="cuda")
        net.train_forward_outputs(encT, S, out[:S], rad[:S])
        return out, rad

    assert (N_BASE + 63) // 64 <= 4 * cus
    out0, rad0 = run(N_BASE)
    torch.cuda.synchronize()
    assert bool((out0[N_BASE:] == -5.0).all()) and bool((rad0[N_BASE:] == -5.0).all())
    out0, rad0 = out0[:N_BASE], rad0[:N_BASE]
    assert torch.equal(rad0, out0[:, :4].float()) and float(out0.float().std()) > 1e-3
    S = (7 * 4 * PER_CU * cus // 2) * 64 + 37
    out, rad = run(S)
    tag = f"train_forward_outputs, {depth} x 64, E = {E}, {S} samples"
    _assert_copies(torch, out, out0, S, -5.0, tag, 64, 4 * PER_CU * cus)
    _assert_copies(torch, rad, rad0, S, -5.0, tag + " (radiance)", 64, 4 * PER_CU * cus)
