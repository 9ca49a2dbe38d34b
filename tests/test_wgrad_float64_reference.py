"""What the per-element bound of tests/_wgrad_float64.py lets through and what it catches, on the CPU.

A numpy fp32 emulation of the recomputing weight-gradient kernels' block-wise sums (W.emulate: persistent blocks, 256-sample
tiles, 16-sample k-steps, one partial per block) stays inside bound = u |ref| + k u mag at the shapes
tests/test_gpu_wgrad_float64.py runs on the device, in both modes; every defect those kernels can have and a norm-relative
bar cannot see -- a sample, a wave's 64 samples, a tile too many or too few, a quadrant in the wrong place, a missing k-step, the
wrong layer's input, a non-zero padding row, an unlisted segment, a lost accumulate, a NaN -- puts elements outside it.
The CU count of the device is a parameter here: 256 (a whole MI355X) for the sizes derived from it."""
import numpy as np
import pytest

import _wgrad_float64 as W

CUS = 256


def _case(width, L, E, n, seed):
    """Tensors shaped and scaled like a training step's: X_0 uniform encodings, X_l post-ReLU (half of it +0), dZ_l masked by
    the layer's own activation, dZ_L with rows 4..15 zero.  Returns (dZ list, X list), layers 0..L, fp16 [features][n]."""
    rng = np.random.default_rng(seed)
    X = [rng.uniform(-1, 1, (E, n)).astype(np.float16)]
    X += [np.maximum(rng.standard_normal((width, n)) * 0.5, 0).astype(np.float16) for _ in range(L)]
    dZ = [((rng.standard_normal((width, n)) * 0.01) * (X[l + 1] > 0)).astype(np.float16) for l in range(L)]
    dzL = np.zeros((16, n), np.float16)
    dzL[:4] = (rng.standard_normal((4, n)) * 0.01).astype(np.float16)
    return dZ + [dzL], X


def _k(n, grid, listed=None):
    return W.k_recompute(W.n_tiles_of(n, listed), grid)


# ------------------------------------------------------------------------------------------------------- the derivation's own numbers
def test_k_and_the_grids_follow_the_launchers():
    assert W.k_recompute(3, 3) == 32 + 3 + 2
    n = 256 * (2 * CUS + 35) + 37                         # 140,069 at 256 CUs: 35 blocks run three tiles, the last one ragged
    tiles = W.n_tiles_of(n)
    assert n == 140_069 and tiles == 2 * CUS + 36 and W.persistent_grid(tiles, CUS) == CUS and _k(n, CUS) == 354
    assert not W.all_pass_used(tiles, CUS, False) and not W.all_pass_used(tiles, CUS, True)
    n = 256 * (4 * CUS + 5) + 37
    assert W.all_pass_used(W.n_tiles_of(n), CUS, False) and W.all_pass_used(W.n_tiles_of(n), CUS, True)
    assert W.all_pass_grid(CUS, False) == 72 and W.all_pass_grid(CUS, True) == 64        # 9 : 11 : 12 and 8 : 11 : 13 of 32 slots x 8 XCDs
    # the smallest share's k covers the larger shares'
    for folded, shares in ((False, (72, 88, 96)), (True, (64, 88, 104))):
        k = W.k_recompute(W.n_tiles_of(n), W.all_pass_grid(CUS, folded))
        assert all(W.k_recompute(W.n_tiles_of(n), g) <= k for g in shares)
    assert W.n_tiles_of(3200, listed=9) == 2 and W.n_tiles_of(3200, listed=8) == 1
    assert W.layer_sizes(64, 2, 48) == [(64, 48), (64, 64), (16, 64)]


# ------------------------------------------------------------------------------------------------------- a faithful kernel passes
FUSED = [(L, E, 700) for L in (1, 2, 3, 4) for E in (16, 32, 48, 64)] + [(L, E, n) for L, E in ((1, 16), (2, 48), (4, 64)) for n in (5, 256)]
FUSED += [(2, 48, 1536)]


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("L,E,n", FUSED)
def test_faithful_emulation_is_inside_the_bound_fused_shapes(L, E, n, deterministic):
    dZ, X = _case(64, L, E, n, seed=L * 100 + E + n)
    grid = W.persistent_grid(W.n_tiles_of(n), CUS)
    ref, mag = W.reference(dZ, X)
    res = W.check(W.emulate_layers(dZ, X, grid, deterministic=deterministic), ref, mag, _k(n, grid), W.layer_sizes(64, L, E),
                  det_atomics=grid if deterministic else None)
    print(W.lines(f"emulation 64x{L} E{E} n{n} det={deterministic}", res))
    assert res.bad == 0 and max(res.worst) <= 1


@pytest.mark.parametrize("width,L,E,n,grid", [(64, 1, 16, 256 * (2 * CUS + 35) + 37, CUS), (64, 4, 64, 256 * (2 * CUS + 35) + 37, CUS),
                                              (128, 8, 112, 5, 1), (128, 8, 112, 700, 3), (128, 1, 112, 256 * (2 * CUS + 35) + 37, CUS),
                                              (128, 1, 112, 256 * (4 * CUS + 5) + 37, 72), (128, 1, 112, 256 * (4 * CUS + 5) + 37, 64)])
def test_faithful_emulation_is_inside_the_bound_deep_loops_and_lean_shapes(width, L, E, n, grid):
    """Three tiles deep over a whole chip, and the single launch's smallest share (15 and 17 tiles per block)"""
    dZ, X = _case(width, L, E, n, seed=width + L + E)
    ref, mag = W.reference(dZ, X)
    res = W.check(W.emulate_layers(dZ, X, grid), ref, mag, _k(n, grid), W.layer_sizes(width, L, E))
    print(W.lines(f"emulation {width}x{L} E{E} n{n} grid{grid}", res))
    assert res.bad == 0 and max(res.worst) <= 1


def _listed(P, count, seed):
    rng = np.random.default_rng(seed)
    live = np.zeros(P, bool)
    live[[0, P - 1][:count]] = True
    rest = np.setdiff1d(np.arange(P), np.nonzero(live)[0])
    live[rng.choice(rest, count - int(live.sum()), replace=False)] = True
    return live


@pytest.mark.parametrize("count", [1, 8, 9, 31])
def test_faithful_emulation_is_inside_the_bound_live_form(count):
    """The reference of the live form is the list-free product with dZ zeroed on the unlisted segments"""
    P, L, E = 100, 2, 48
    live = _listed(P, count, seed=count)
    dZ, X = _case(64, L, E, 32 * P, seed=count)
    zeroed = [np.where(np.repeat(live, 32)[None, :], d, np.float16(0)) for d in dZ]
    ref, mag = W.reference(zeroed, X)
    tiles = W.n_tiles_of(32 * P, listed=count)
    grid = W.persistent_grid(tiles, CUS)
    got = W.emulate_layers(dZ, X, grid, live_list=np.nonzero(live)[0])
    res = W.check(got, ref, mag, W.k_recompute(tiles, grid), W.layer_sizes(64, L, E))
    assert res.bad == 0 and max(res.worst) <= 1


def test_the_fixed_point_term_is_what_tiny_deterministic_gradients_need():
    """One block, five samples, gradients near 2^-20: the deterministic mode's rounding of the partial to 2^-40 is larger than
    k u mag; inside the bound with the 2^-41 term, outside without, and the default mode needs none"""
    L, E, n = 2, 48, 5
    dZ, X = _case(64, L, E, n, seed=21)
    dZ = [(d.astype(np.float32) * 2.0 ** -13).astype(np.float16) for d in dZ]
    ref, mag = W.reference(dZ, X)
    k, sizes = _k(n, 1), W.layer_sizes(64, L, E)
    det = W.emulate_layers(dZ, X, 1, deterministic=True)
    assert W.check(det, ref, mag, k, sizes, det_atomics=1).bad == 0
    assert W.check(det, ref, mag, k, sizes).bad > 0
    assert W.check(W.emulate_layers(dZ, X, 1), ref, mag, k, sizes).bad == 0


# ------------------------------------------------------------------------------------------------------- planted defects
class Planted:
    """One model, its reference, and the faithful result; n = 700 on two blocks (block 0 runs tiles 0 and 2, the ragged one) or
    140,069 on 256 (three tiles deep, k = 354: the bound at its widest)."""

    def __init__(self, L, E, n, grid, seed):
        self.L, self.E, self.n, self.grid = L, E, n, grid
        self.dZ, self.X = _case(64, L, E, n, seed)
        self.ref, self.mag = W.reference(self.dZ, self.X)
        self.k = _k(n, grid)
        self.sizes = W.layer_sizes(64, L, E)
        self.tiles = W.n_tiles_of(n)

    def run(self, dZ=None, X=None, **kw):
        return W.emulate_layers(self.dZ if dZ is None else dZ, self.X if X is None else X, self.grid, **kw)

    def bad(self, got, **kw):
        return W.check(got, self.ref, self.mag, self.k, self.sizes, **kw).bad

    def without_samples(self, cols):
        dZ = [d.copy() for d in self.dZ]
        for d in dZ:
            d[:, cols] = 0
        return dZ


@pytest.fixture(scope="module", params=[(2, 48, 700, 2), (1, 16, 256 * (2 * CUS + 35) + 37, CUS)], ids=["n700", "n140069"])
def planted(request):
    L, E, n, grid = request.param
    p = Planted(L, E, n, grid, seed=7)
    p.good = p.run()
    assert p.bad(p.good) == 0
    return p


def test_the_last_ragged_sample_dropped(planted):
    p = planted
    assert p.bad(p.run(dZ=p.without_samples(slice(p.n - 1, p.n)))) > 0


def test_one_wave_of_the_last_tile_dropped(planted):
    """The last tile's first wave (its third one stops inside a column tile, the fourth is empty)"""
    p = planted
    t0 = (p.tiles - 1) * 256
    assert p.bad(p.run(dZ=p.without_samples(slice(t0, t0 + 64)))) > 0


def test_one_tile_summed_twice(planted):
    p = planted
    sched = W.block_schedule(p.tiles, p.grid)
    sched[1] = sched[1] + sched[1][-1:]
    assert p.bad(p.run(schedule=sched)) > 0


def test_one_tile_skipped_after_the_first_loop_iteration(planted):
    p = planted
    sched = W.block_schedule(p.tiles, p.grid)
    assert len(sched[0]) >= 2
    sched[0] = sched[0][:1] + sched[0][2:]
    assert p.bad(p.run(schedule=sched)) > 0


@pytest.mark.parametrize("how", ["transposed", "swapped"])
def test_one_quadrant_in_the_wrong_place(planted, how):
    """Layer 1 where there is one (64 x 64), else the output layer's neighbour columns: a 32 x 32 quadrant transposed in place, or
    exchanged with the quadrant beside it"""
    p = planted
    got = p.good.copy()
    if p.L >= 2:
        g = got[64 * p.E:64 * p.E + 4096].reshape(64, 64)
        if how == "transposed":
            g[32:, :32] = g[32:, :32].T.copy()
        else:
            g[:32, :32], g[:32, 32:] = g[:32, 32:].copy(), g[:32, :32].copy()
    else:
        g = got[64 * p.E:].reshape(16, 64)
        if how == "transposed":
            g[:16, :16] = g[:16, :16].T.copy()
        else:
            g[:, :32], g[:, 32:] = g[:, 32:].copy(), g[:, :32].copy()
    assert p.bad(got) > 0


def test_layer_0_one_k_step_short_at_48_features():
    p = Planted(2, 48, 700, 3, seed=11)
    X = [x.copy() for x in p.X]
    X[0][32:] = 0                                          # the third 16-feature k-step of the recomputed input never read
    assert p.bad(p.run()) == 0 and p.bad(p.run(X=X)) > 0


def test_input_taken_from_the_layer_before():
    p = Planted(3, 64, 700, 3, seed=12)
    X = list(p.X)
    X[2] = p.X[1]
    assert p.bad(p.run(X=X)) > 0


def test_output_rows_4_to_15_not_zero(planted):
    p = planted
    got = p.good.copy()
    assert not got[-16 * 64:].reshape(16, 64)[4:].any()
    got[-1] = 1e-30                                        # bound there is exactly zero: nothing but zero is inside it
    assert p.bad(got) == 1


def test_an_unlisted_segment_included():
    P, L, E = 100, 2, 48
    live = _listed(P, 31, seed=3)
    dZ, X = _case(64, L, E, 32 * P, seed=13)
    ref, mag = W.reference([np.where(np.repeat(live, 32)[None, :], d, np.float16(0)) for d in dZ], X)
    sizes = W.layer_sizes(64, L, E)
    lst = np.nonzero(live)[0]
    tiles = W.n_tiles_of(32 * P, listed=lst.size)
    k = W.k_recompute(tiles, tiles)
    assert W.check(W.emulate_layers(dZ, X, tiles, live_list=lst), ref, mag, k, sizes).bad == 0
    other = np.nonzero(~live)[0][0]
    wrong = np.sort(np.append(lst, other))
    assert W.check(W.emulate_layers(dZ, X, tiles, live_list=wrong), ref, mag, k, sizes).bad > 0
    # a slot past the list reading segment 0 (what the kernels fetch there) and NOT adding zeros
    assert W.check(W.emulate_layers(dZ, X, tiles, live_list=np.append(lst, 0)), ref, mag, k, sizes).bad > 0


@pytest.mark.parametrize("deterministic", [False, True])
def test_overwrite_in_place_of_accumulate(planted, deterministic):
    p = planted
    pre = np.random.default_rng(5).standard_normal(p.ref.size).astype(np.float32)
    acc = p.run(pre=pre, deterministic=deterministic)
    assert p.bad(acc, pre=pre, grid=p.grid, det_atomics=p.grid if deterministic else None) == 0
    if deterministic:                                      # the fold adds the exact sum once: bit for bit pre + (run into zeros)
        np.testing.assert_array_equal(acc, pre + p.run(deterministic=True))
    assert p.bad(p.good, pre=pre, grid=p.grid) > 0         # the gradient alone where pre + gradient belongs


def test_a_nan_or_inf_in_one_element(planted):
    p = planted
    for v in (np.nan, np.inf, -np.inf):
        got = p.good.copy()
        got[got.size // 3] = v
        res = W.check(got, p.ref, p.mag, p.k, p.sizes)
        assert res.bad == 1 and max(res.worst) == np.inf and res.first == got.size // 3
