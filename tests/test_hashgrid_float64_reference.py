"""The float64 restatement of the hash grid (tests/_hashgrid_float64.py) without a GPU -- but with the project BUILT: the oracle
fixture compiles the CPU oracle, and test_geometry_equals_the_library_and_the_oracle calls rtxn_hashgrid_create (host code of
librtxn.so), so on a tree whose library was never built that test fails with RtxnError; it does not skip.

tests/test_gpu_hashgrid_float64.py holds the encode and scatter kernels to derived bounds, per element and per entry, over the
configurations rtxn_hashgrid_create accepts.  Here the same checkers run on the CPU:
  * the restatement's geometry equals the library's and the oracle's, level by level, on every configuration of the sweep, and
    its float32 level scales are the C library's exp2f / log2f;
  * the oracle's encode and scatter stay inside the bounds the GPU tests use (a half-ulp bound sits just under 1), on the same
    inputs -- lattice points, +-1, the float32 neighbours of a cell face included;
  * the restatement reproduces tests/golden/kat_north_star.npz, the one closed-form file written before it;
  * nine defects of the kinds a hash grid can have, seeded one at a time into a stand-in "kernel", each fail the SAME
    assertions the GPU test makes, on at least one configuration of the sweep -- and the faithful stand-in passes them all;
  * a NaN or an infinity anywhere in a kernel's output -- an encoded element, a touched table entry, an untouched one -- fails
    those assertions too, and an exact zero of the reference is held to 2^-25, not to the ulp of 1;
  * the direction features' bound needs its fp32 phase term: an exact sine behind the kernel's fp32 "+ 1/4 turn" misses the bare
    fp16 ulp where the cosine crosses zero.
"""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest

import _hashgrid_float64 as H

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = ["%dx%d-T%d-b%d-s%g" % c for c in H.SWEEP]


def _samples(oracle, levels, seed, stype=0):
    sp, ep, view = H.case_segments(levels, seed)
    P = sp.shape[0]
    x, _ = oracle.sample(sp, ep, view, np.ones(P, np.int32), np.arange(P, dtype=np.int32), stype)
    if stype == 0:
        assert np.array_equal(x[::32, :3], sp)             # REGULAR: sample 0 is the start point, special points included
    return x


@pytest.mark.parametrize("cfg", H.SWEEP, ids=IDS)
def test_geometry_equals_the_library_and_the_oracle(oracle, cfg):
    L, F, T, base, s = cfg
    levels = H.geometry(L, T, base, s)
    # the oracle, level by level: its parameter count with the first l levels only
    assert [oracle.hg_n_params(oracle.hg_cfg(l, F, T, base, s)) for l in range(1, L + 1)] == H.level_offsets(levels, F)[1:]
    from rtx_nerf_amd import api                           # rtxn_hashgrid_create is host code
    hg = api.HashGrid(L, F, T, base, s, n_dir_freqs=0)
    assert [hg.level_offset(l) for l in range(L + 1)] == H.level_offsets(levels, F)
    assert hg.n_params() == H.n_entries(levels) * F
    first_hashed = next((lv.offset * F for lv in levels if lv.hashed), H.n_entries(levels) * F)
    assert hg.hashed_offset() == first_hashed
    # float32 scales: the C library's exp2f / log2f give what the restatement takes as correctly rounded
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.exp2f.restype = m.log2f.restype = ctypes.c_float
    m.exp2f.argtypes = m.log2f.argtypes = [ctypes.c_float]
    for l, lv in enumerate(levels):
        c = np.float32(m.exp2f(np.float32(l) * np.float32(m.log2f(s)))) * np.float32(base) - np.float32(1.0)
        assert float(c) == lv.scale, (l, float(c), lv.scale)


def test_sweep_covers_what_it_is_there_for():
    geo = {c: H.geometry(c[0], c[2], c[3], c[4]) for c in H.SWEEP}
    assert geo[H.SWEEP[0]][-1].res == 7007 and 7007 ** 3 > 2 ** 32          # 16 * 1.5^15 = 7006.3
    assert all(lv.hashed and lv.size == 16 for lv in geo[(4, 2, 4, 8, 2.0)])
    assert not any(lv.hashed for c in [(3, 2, 24, 2, 2.0), (2, 2, 24, 2, 2.0)] for lv in geo[c])
    assert all(lv.res ** 3 == lv.size == 4096 and not lv.hashed for lv in geo[(2, 2, 12, 16, 1.0)])
    assert geo[(3, 1, 10, 1, 2.0)][0].res == 1 and geo[(3, 1, 10, 1, 2.0)][0].scale == 0.0
    assert {lv.hashed for lv in geo[(5, 1, 10, 4, 1.7)]} == {False, True}
    assert geo[(6, 2, 12, 4, 1.6)][1].scale == float(np.float32(5.4000001))
    # the near-face switch is exercised: the nextafter points are nearer than tau to a face of their level
    for c, levels in geo.items():
        sp, _, _ = H.case_segments(levels, 1)
        near = H.near_face(levels, sp)
        k = 64
        for l, lv in enumerate(levels):
            if lv.scale > 0:
                assert near[k:k + 3, l].all(), (c, l)
                k += 3


@pytest.mark.parametrize("cfg", H.SWEEP, ids=IDS)
def test_oracle_encode_and_scatter_stay_inside_the_gpu_bounds(oracle, cfg, capsys):
    L, F, T, base, s = cfg
    levels = H.geometry(L, T, base, s)
    ocfg = oracle.hg_cfg(L, F, T, base, s)
    table = H.case_table(levels, F, L)
    ndf = 4
    for stype in (0, 3):
        x = _samples(oracle, levels, L + F, stype)
        enc = H.encode(levels, F, table, x)
        got = oracle.encode_hg(ocfg, ndf, table, x)
        ratio, equal, bad = H.check_encode(enc, got[:, :L * F])
        dref, dbound = H.directions(ndf, x[:, 3:5])
        derr = np.abs(got[:, L * F:L * F + 4 * ndf].astype(np.float64) - dref)
        assert np.all(derr <= dbound)
        assert np.all(got[:, L * F + 4 * ndf:] == 1.0)
        d, zeroed = H.case_gradient(levels, F, x, L + stype, H.case_live(L))      # the GPU test's gradient, dead segments and all
        sc = H.scatter(levels, F, x, d)
        sratio, sbad = H.check_scatter(sc, oracle.hg_backward(ocfg, x, d), "float64")
        with capsys.disabled():
            print(f"\noracle {IDS[H.SWEEP.index(cfg)]} stype {stype}: encode err/bound {ratio:.3f} (equal to fp16(ref) {equal:.4f}, near-face "
                  f"{enc.near.mean():.4f}), scatter err/bound {sratio:.3f}, zeroed {zeroed:.4f}")
        assert bad == 0 and ratio <= 1.0, (ratio, bad)
        assert sbad == 0 and sratio <= 1.0, (sratio, sbad)
        assert zeroed <= 0.02
        assert np.count_nonzero(sc.sum) > 0 and equal > 0.8


def test_restatement_reproduces_the_closed_form_golden_file():
    NS = np.load(os.path.join(HERE, "golden", "kat_north_star.npz"))
    L, F, T, base = (int(v) for v in NS["hg_cfg"])
    levels = H.geometry(L, T, base, float(NS["hg_scale"][0]))
    assert [lv.size for lv in levels] == NS["hg_level_sizes"].tolist()
    enc = H.encode(levels, F, NS["hg_table"], NS["hg_points"])
    # The file's generator took its float32 level scales from numpy's float32 exp2, which is an ulp off the C library's exp2f on
    # some levels (here: the restatement's scales are asserted equal to the C library's above).  An ulp of the scale moves pos by
    # at most scale 2^-23 per axis -- inside the positional term of the bound, which is therefore the whole allowance here.
    # Level 0's scale (base - 1) is exact either way: there only two float64 sums in different orders remain.
    np.testing.assert_allclose(enc.ref[:, :F], NS["hg_enc"][:, :F], rtol=0, atol=1e-12)
    assert np.all(np.abs(enc.ref - NS["hg_enc"]) <= enc.pos + 1e-12)
    assert H.check_encode(enc, NS["hg_enc"].astype(np.float16))[2] == 0


# ---------------------------------------------------------------------------------------------------------- seeded defects
def _standin(cfg, defect, x):
    """What a kernel with `defect` would write: (encoded fp16 [n, L * F], table gradient float64), computed with the defective
    restatement on the true table layout."""
    L, F, T, base, s = cfg
    levels = H.geometry(L, T, base, s)
    bad = H.geometry(L, T, base, s, defect)
    table = H.case_table(levels, F, L)
    d, _ = H.case_gradient(levels, F, x, L)
    got = H.to_half(H.encode(bad, F, table, x, defect).ref, defect)
    grad = np.zeros(H.n_entries(levels) * F)
    sc = H.scatter(bad, F, x, d, defect)
    k = min(grad.size, sc.sum.size)
    grad[:k] = sc.sum[:k]
    return H.encode(levels, F, table, x), got, H.scatter(levels, F, x, d), grad


SMALL = [c for c in H.SWEEP if c[0] * c[1] <= 32 and c[2] <= 14]      # the seeded runs need no 12.6 M-entry tables


@pytest.fixture(scope="module")
def points(oracle):
    return {c: _samples(oracle, H.geometry(c[0], c[2], c[3], c[4]), c[0] + c[1]) for c in SMALL}


def test_faithful_standin_passes(points):
    for c in SMALL:
        enc, got, sc, grad = _standin(c, None, points[c])
        ratio, equal, bad = H.check_encode(enc, got)
        assert bad == 0 and equal == 1.0
        assert H.check_scatter(sc, grad.astype(np.float32), "fp32")[1] == 0


def test_non_finite_output_fails_the_gpu_assertions(points):
    """One NaN, one infinity: in an encoded element, in a table entry the reference touches and in one it leaves at zero.  Every
    form's checker counts it (a comparison with NaN is False, so the checkers count what is NOT inside its bound)."""
    c = (6, 2, 12, 4, 1.6)
    enc, got, sc, grad = _standin(c, None, points[c])
    touched, untouched = np.flatnonzero(sc.n > 0), np.flatnonzero(sc.n == 0)
    assert touched.size and untouched.size
    for poison in (np.nan, np.inf, -np.inf):
        g = got.copy()
        g[7, 1] = poison
        ratio, _, bad = H.check_encode(enc, g)
        assert bad == 1 and not ratio <= 1.0
        for where in (touched[touched.size // 2], untouched[untouched.size // 2]):
            for form, dtype in (("fp32", np.float32), ("fp16", np.float16), ("float64", np.float32), ("deterministic", np.float32)):
                v = grad.astype(dtype)
                assert H.check_scatter(sc, v, form, n_atomics=8 * points[c].shape[0])[1] == 0
                v[where] = poison
                assert H.check_scatter(sc, v, form, n_atomics=8 * points[c].shape[0])[1] >= 1, (poison, where, form)
    enc_all = H.check_encode(enc, np.full_like(got, np.nan))
    assert enc_all[2] == got.size
    assert H.check_scatter(sc, np.full(grad.size, np.nan, np.float32), "fp32")[1] == grad.size


def test_half_ulp_of_an_exact_zero_is_the_subnormal_floor():
    ref = np.array([0.0, -0.0, 2.0 ** -26, 2.0 ** -24, 2.0 ** -14, 0.75, -1.0, 1.5])
    want = np.array([2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -12, 2.0 ** -11, 2.0 ** -11])
    assert np.array_equal(H.half_ulp16(ref), want)
    ref16 = np.array([0.0, 6e-8, 1e-4, 0.3, 0.9999, 1.0, 1000.0])      # half the gap to the next fp16, by numpy's own spacing
    assert np.array_equal(H.half_ulp16(ref16.astype(np.float16).astype(np.float64)), np.spacing(ref16.astype(np.float16)).astype(np.float64) / 2)


def test_direction_bound_needs_its_fp32_phase_term():
    """sin_turns() adds the quarter turn of the cosines in fp32.  Give it an exact sine behind that one rounding: the result stays
    inside the bound of directions(), the sines (no addition) inside 1 fp16 ulp alone -- half an ulp in fact --, and the cosines
    leave the bare ulp behind at their zero crossings, where an ulp of the reference is smaller than 2 pi 2^-24."""
    rng = np.random.default_rng(5)
    dirs = rng.uniform(-3.1, 3.1, (4000, 2)).astype(np.float32)
    dirs[:3] = [(0.0, 0.0), (0.5, -0.5), (1.0, 3.0)]                     # exact zeros of the sine and of the cosine
    # beside a zero of the lowest octave's cosine, an odd number of fp32 steps away: x / 2 = 3/4 + k 2^-24 is exact, + 1/4 is not
    # (fp32 is spaced 2^-23 apart above 1), and cos(pi x) = sin(k pi 2^-23) is smaller than the 2 pi 2^-24 the rounding moves it by
    k = np.arange(-9, 10, 2)
    dirs[3:3 + k.size, 0] = (1.5 + k * 2.0 ** -23).astype(np.float32)
    dirs[3:3 + k.size, 1] = (0.5 + k * 2.0 ** -24).astype(np.float32)   # the other zero: 1/4 + k 2^-25, + 1/4 is spaced 2^-24
    assert np.array_equal(dirs[3:3 + k.size, 0].astype(np.float64), 1.5 + k * 2.0 ** -23)
    ndf = 12
    ref, bound = H.directions(ndf, dirs)
    got = H.directions_fp32_phase(ndf, dirs).astype(np.float64)
    err = np.abs(got - ref)
    bare = err / H.directions_bare_bound(ref)
    cos = np.tile([False, True], 2 * ndf)
    print(f"\nexact sine behind the fp32 phase: err / bound {float((err / bound).max()):.3f}; against 1 fp16 ulp alone: sines "
          f"{float(bare[:, ~cos].max()):.3f}, cosines {float(bare[:, cos].max()):.3f} ({int((bare > 1).sum())} of {bare.size} values above)")
    assert np.all(err <= bound)
    assert bare[:, ~cos].max() <= 0.5 + 1e-9
    assert bare[:, cos].max() > 1.0
    worst = np.unravel_index(np.argmax(bare), bare.shape)
    assert abs(ref[worst]) < 2.0 ** -10                                  # at a zero crossing, nowhere else


def test_packed_fp16_bound_needs_its_subnormal_floor(points):
    """The correctly rounded fp16 of the exact float64 sum -- the best any fp16 accumulation can do -- stays inside the packed
    fp16 bound, and misses the same form WITHOUT the 2^-25 per rounding on some entry: fp16 is spaced 2^-24 apart below 2^-14."""
    missed = 0
    for c in SMALL:
        L, F, T, base, s = c
        levels = H.geometry(L, T, base, s)
        d, _ = H.case_gradient(levels, F, points[c], L)
        sc = H.scatter(levels, F, points[c], d)
        best = sc.sum.astype(np.float16)
        assert H.check_scatter(sc, best, "fp16")[1] == 0
        missed += H.check_scatter(sc, best, "fp16 without the subnormal floor")[1]
    assert missed > 0


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_seeded_defect_fails_the_gpu_assertions(points, defect):
    caught_enc, caught_sc = [], []
    for c in SMALL:
        enc, got, sc, grad = _standin(c, defect, points[c])
        if H.check_encode(enc, got)[2] > 0:
            caught_enc.append(c)
        if H.check_scatter(sc, grad.astype(np.float32), "fp32")[1] > 0:
            caught_sc.append(c)
    assert caught_enc, f"{defect}: no configuration's encode assertion fails"
    if defect != "rtz":                                     # a conversion defect of the encoder's output stage only
        assert caught_sc, f"{defect}: no configuration's scatter assertion fails"
