"""The hash-grid kernels against the float64 restatement of tests/_hashgrid_float64.py, per encoded element and per table entry,
over the configurations rtxn_hashgrid_create accepts (the sweep of that module: F = 1, 2, 4, 8; odd level counts; grids that
are all hashed, all dense, exactly full (res^3 == 2^T), flat (per_level_scale 1), one cell wide (base_resolution 1)).  The
bounds are DERIVED there, not measured: half an fp16 ulp + the fp32 arithmetic + the fp32 rounding of the position for the
encoders; the fp32 / fp16 atomics' roundings + the position for the scatter.  No flat tolerance anywhere.  The checkers count
what is NOT inside its bound, so a NaN or an infinity fails like any other value (shown on the CPU by
test_non_finite_output_fails_the_gpu_assertions), and every test asserts the largest err / bound <= 1 besides.
  * encode, encode_segments (REGULAR, MIDPOINT_WORLD): hash features inside the bound, direction features inside theirs, padding
    features exactly 1, padded columns exactly 0, guard rows around the buffer untouched; for F = 2 the general kernel (a table
    view offset by one entry, 4-byte aligned only) equals the two-feature kernel bit for bit;
  * backward, backward_segments (both sampling modes) and the live-list form: every entry inside the bound, entries the
    reference leaves at zero exactly zero (guard words around the buffer untouched); backward_mixed where it applies; the
    deterministic form with its fixed-point bound;
  * hashmlp_forward_segments == the staged chain bit for bit wherever hashmlp_supported holds.
What the MI355X measured (largest err / bound per configuration and form, the share of outputs equal to fp16(ref), the share
of (sample, level) pairs zeroed for nearness to a face): profiles/r16/hashgrid_float64.txt."""
import numpy as np
import pytest

import _hashgrid_float64 as H

pytestmark = pytest.mark.gpu

N_DIR = [4, 0, 12, 4, 0, 12, 4, 12, 0, 4]                   # direction octaves, spread over the sweep (E <= 64 where F = 2, L even)
CASES = [c + (n,) for c, n in zip(H.SWEEP, N_DIR)]
IDS = ["%dx%d-T%d-b%d-s%g-d%d" % c for c in CASES]
SENT16, SENT32 = -7.75, -7.75
P = 300


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(autouse=True)
def _restore_default_mode(gpu):
    yield
    from rtx_nerf_amd import api
    api.set_deterministic(None, None)


def _case(torch, api, case):
    """Grid, table (aligned, and a view offset by one entry), segments: what every test of a configuration needs, and no more --
    the float64 arrays are built by the test that uses them and die with it (the bench grid's are ~100 MB each)."""
    L, F, T, base, s, ndf = case
    levels = H.geometry(L, T, base, s)
    hg = api.HashGrid(L, F, T, base, s, n_dir_freqs=ndf)
    assert [hg.level_offset(l) for l in range(L + 1)] == H.level_offsets(levels, F)        # geometry: equal, not tolerated
    assert hg.encoded_width() == -(-(L * F + 4 * ndf) // 16) * 16
    table = H.case_table(levels, F, L)
    tab_d = torch.empty(table.size + 2, dtype=torch.float16, device="cuda")                 # [2:]: 4-byte aligned only
    aligned = _dev(torch, table)
    tab_d[2:] = aligned
    assert aligned.data_ptr() % 8 == 0 and tab_d[2:].data_ptr() % 8 == 4
    sp, ep, view = H.case_segments(levels, L + F, P)
    seg = tuple(_dev(torch, a) for a in (sp, ep, view))
    return dict(levels=levels, hg=hg, table=table, aligned=aligned, offset_view=tab_d[2:], seg=seg, np_seg=(sp, ep, view))


def _positions(torch, api, c, stype):
    """The sampler's own positions of the case's segments: (device [32 P, 5], numpy)"""
    ones, idx = _dev(torch, np.ones(P, np.int32)), _dev(torch, np.arange(P, dtype=np.int32))
    samples = torch.zeros((32 * P, 5), device="cuda")
    t = torch.zeros(32 * P, device="cuda")
    api.launchSampler(*c["seg"], t, samples, P, 8, ones, idx, stype)
    x = samples.cpu().numpy()
    if stype == 0:
        assert np.array_equal(x[::32, :3], c["np_seg"][0])  # sample 0 of a REGULAR segment IS its start: the special points arrive
    return samples, x


def _guarded(torch, rows, cols, dtype, fill):
    """[rows, cols] inside a buffer with one guard row of `fill` before and behind it"""
    buf = torch.full((rows + 2, cols), fill, dtype=dtype, device="cuda")
    return buf, buf[1:rows + 1]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_encoders_match_float64_per_element(gpu, case):
    torch = gpu
    from rtx_nerf_amd import api
    L, F, T, base, s, ndf = case
    c = _case(torch, api, case)
    hg, S = c["hg"], 32 * P
    E, Sp, nh = hg.encoded_width(), api.padded_samples(32 * P), L * F
    sp_d, ep_d, sv_d = c["seg"]

    def run(form, stype, table, samples):
        buf, encT = _guarded(torch, E, Sp, torch.float16, SENT16)
        if form == "plain":
            hg.encode(table, samples, encT)
        else:
            hg.encode_segments(table, sp_d, ep_d, sv_d, P, stype, encT)
        torch.cuda.synchronize()
        assert bool((buf[0] == SENT16).all()) and bool((buf[-1] == SENT16).all()), f"{form}: wrote outside encT"
        return encT.cpu().numpy()

    for stype in (0, 3):
        samples, x = _positions(torch, api, c, stype)
        enc = H.encode(c["levels"], F, c["table"], x)
        dref, dbound = H.directions(ndf, x[:, 3:5])
        first = None
        for form in ("plain", "segments"):
            got = run(form, stype, c["aligned"], samples)
            assert np.isfinite(got.astype(np.float32)).all(), (form, stype)
            ratio, equal, bad = H.check_encode(enc, got[:nh, :S].T)
            print(f"measured encode {IDS[CASES.index(case)]} {form} stype {stype}: err / bound {ratio:.3f}, equal to fp16(ref) {equal:.4f}, "
                  f"near-face samples {enc.near.mean():.4f}")
            assert bad == 0 and ratio <= 1.0, (form, stype, ratio, bad)
            derr = np.abs(got[nh:nh + 4 * ndf, :S].T.astype(np.float64) - dref)
            if ndf:
                bare = derr / H.directions_bare_bound(dref)
                print(f"measured directions {form} stype {stype}: err / bound {float((derr / dbound).max()):.3f} "
                      f"(against 1 fp16 ulp alone {float(bare.max()):.3f}, {int((bare > 1).sum())} of {bare.size} values above)")
            assert np.all(derr <= dbound), (form, stype, float((derr / dbound).max()))
            assert np.all(got[nh + 4 * ndf:, :S] == 1.0) and np.all(got[:, S:] == 0.0)
            if first is None:
                first = got
            else:
                np.testing.assert_array_equal(got.view(np.uint16), first.view(np.uint16))     # the folded sampler == the sampler
            if F == 2:      # the general kernel on two features: selected by the table's alignment, bit-identical by claim
                other = run(form, stype, c["offset_view"], samples)
                np.testing.assert_array_equal(other.view(np.uint16), got.view(np.uint16))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scatter_matches_float64_per_entry(gpu, case):
    torch = gpu
    from rtx_nerf_amd import api
    L, F, T, base, s, ndf = case
    c = _case(torch, api, case)
    hg, levels, S = c["hg"], c["levels"], 32 * P
    E, Sp, nh, NP = hg.encoded_width(), api.padded_samples(32 * P), L * F, hg.n_params()
    lo = hg.hashed_offset()
    sp_d, ep_d, sv_d = c["seg"]
    live = H.case_live(L, P)                                # 30 % of the segments dead; the special points stay in
    dout = torch.zeros((S, 4), dtype=torch.float16, device="cuda")
    dout.view(P, 32, 4)[_dev(torch, live), 0, 0] = 1.0
    ws = api.live_segments_workspace(P)
    api.live_segments(dout, P, P, ws)
    name = IDS[CASES.index(case)]

    def run(form, stype, samples, denc_d, half=False):
        g32 = torch.full((NP + 16,), SENT32, device="cuda")
        d32 = g32[8:8 + NP]
        d32.zero_()
        g16 = d16 = None
        if half:
            g16 = torch.full((NP - lo + 16,), SENT16, dtype=torch.float16, device="cuda")
            d16 = g16[8:8 + NP - lo]
            d16.zero_()
        if form == "plain":
            (hg.backward_mixed(samples, denc_d, d32, d16) if half else hg.backward(samples, denc_d, d32))
        else:
            hg.backward_segments(sp_d, ep_d, P, stype, denc_d, d32, d16, live_ws=ws if form == "live" else None)
        torch.cuda.synchronize()
        for g in (g32, g16):
            if g is not None:
                assert bool((g[:8] == SENT32).all()) and bool((g[-8:] == SENT32).all()), f"{form}: wrote outside the gradient"
        return d32.cpu().numpy(), (d16.cpu().numpy() if half else None)

    for stype in (0, 3):
        samples, x = _positions(torch, api, c, stype)
        d, zeroed = H.case_gradient(levels, F, x, L + stype, live)
        print(f"measured scatter {name} stype {stype}: near-face pairs zeroed {zeroed:.4f}")
        assert zeroed <= 0.02
        sc = H.scatter(levels, F, x, d)
        assert np.count_nonzero(sc.sum) > 0
        denc = np.zeros((E, Sp), np.float16)
        denc[:nh, :S] = d.T
        denc_d = _dev(torch, denc)
        for form in (("plain", "segments", "live") if stype == 0 else ("segments",)):
            g32, _ = run(form, stype, samples, denc_d)
            ratio, bad = H.check_scatter(sc, g32, "fp32")
            print(f"measured scatter {name} {form} stype {stype} fp32: err / bound {ratio:.3f}")
            assert bad == 0 and ratio <= 1.0, (form, stype, ratio, bad)
            if F == 2 and lo < NP:                          # backward_mixed: the hashed levels through packed fp16 atomics
                h32, h16 = run(form, stype, samples, denc_d, half=True)
                assert np.all(h32[lo:] == 0.0)
                cut = lambda a, sl: H.Scattered(*(v[sl] for v in a))
                r32, b32 = H.check_scatter(cut(sc, slice(0, lo)), h32[:lo], "fp32") if lo else (0.0, 0)
                r16, b16 = H.check_scatter(cut(sc, slice(lo, None)), h16, "fp16")
                bare = H.check_scatter(cut(sc, slice(lo, None)), h16, "fp16 without the subnormal floor")
                print(f"measured scatter {name} {form} stype {stype} mixed: err / bound fp32 part {r32:.3f}, fp16 part {r16:.3f} "
                      f"(without the subnormal floor {bare[0]:.3f}, {bare[1]} entries above)")
                assert b32 == 0 and b16 == 0 and r32 <= 1.0 and r16 <= 1.0, (form, stype, r32, r16, b32, b16)
        if stype == 0:                                      # the deterministic form: the fixed-point shadow, then one fold
            shadow = api.deterministic_shadow(NP)
            api.set_deterministic(None, shadow)
            g32, _ = run("plain", stype, samples, denc_d)
            api.set_deterministic(None, None)
            ratio, bad = H.check_scatter(sc, g32, "deterministic", n_atomics=8 * S)
            print(f"measured scatter {name} plain stype {stype} deterministic: err / bound {ratio:.3f}")
            assert bad == 0 and ratio <= 1.0, (ratio, bad)
            assert int(shadow.abs().max()) == 0


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == 2 and c[0] % 2 == 0], ids=[i for c, i in zip(CASES, IDS) if c[1] == 2 and c[0] % 2 == 0])
def test_fused_inference_equals_the_staged_chain(gpu, case):
    """hashmlp_forward_segments against encode_segments + train_forward_outputs on the same segments (lattice, +-1 and face
    points included), bit for bit, on every grid the fused kernel accepts: all hashed, all dense and exactly full among them."""
    torch = gpu
    from rtx_nerf_amd import api, scenes
    L, F, T, base, s, ndf = case
    c = _case(torch, api, case)
    hg = c["hg"]
    E, S = hg.encoded_width(), 32 * P
    net = api.Network(n_neurons=64, n_hidden_layers=2, n_encoded_features=E, output_activation=1)
    assert api.hashmlp_supported(net, hg)
    net.set_params(_dev(torch, scenes.xavier_params_fp16(64, 2, E, seed=L)))
    sp_d, ep_d, sv_d = c["seg"]
    total = torch.tensor([P], dtype=torch.int32, device="cuda")
    for stype in (0, 3):
        rad = torch.full((S + 64, 4), -1.0, dtype=torch.float16, device="cuda")
        api.hashmlp_forward_segments(net, hg, c["aligned"], sp_d, ep_d, sv_d, total, P, rad, stype)
        encT = torch.zeros((E, api.padded_samples(S)), dtype=torch.float16, device="cuda")
        hg.encode_segments(c["aligned"], sp_d, ep_d, sv_d, P, stype, encT)
        out16 = net.train_forward_outputs(encT, S)
        torch.cuda.synchronize()
        got = rad.cpu().numpy()
        np.testing.assert_array_equal(got[:S].view(np.uint16), out16[:, :4].contiguous().cpu().numpy().view(np.uint16))
        assert np.all(got[S:] == -1.0) and np.isfinite(got[:S].astype(np.float32)).all()
