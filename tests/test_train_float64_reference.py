"""The teacher-forced float64 restatements of the training MLP (tests/_train_float64.py) without a GPU.

tests/test_gpu_train_layerwise.py holds every tensor the training kernels leave in the workspace to a derived half-ulp bound.
Here the same checkers run over workspace images built in numpy by a stand-in "kernel" that does what the kernels are meant to
do -- fp32 matrix products, round-to-nearest fp16, ReLU, sign masks, the compact dZ of the live-list form:
  * the faithful stand-in passes every stage, just under the bound (a half-ulp bound sits at 0.9 .. 1);
  * the free-running chain of the same restatements reproduces the CPU oracle within the bars tests/test_gpu_train.py uses;
  * an image packed and decoded round-trips, mask bit order included;
  * seven defects of the kinds these kernels have had, or could have, each fail the SAME assertions the GPU test makes.
"""
import numpy as np
import pytest

import _train_float64 as T
from _mlp_float64 import layers_of
from rtx_nerf_amd import scenes

SHAPES = [(128, 8, 112, 700), (64, 4, 176, 700), (128, 3, 16, 256)]       # (W, L, E, n)


def _rtz(x32):
    """fp32 -> fp16 toward zero"""
    h = x32.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x32)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def _standin(W, L, E, n, sigmoid, seed=0, defect=None, live_list=None, dout_scale=1.0):
    """A workspace image and the tensors around it, as the kernels would leave them.  live_list: the live-list form (acts and
    masks of the listed segments in place, dz / dzL compact, everything else SENTINEL; dencT elsewhere 7)."""
    rng = np.random.default_rng(seed)
    params = scenes.xavier_params_fp16(W, L, E, seed=seed + 1)
    mats = [m.astype(np.float32) for m in layers_of(params, W, L, E)]
    Sp = -(-n // 256) * 256
    encT = np.zeros((E, Sp), np.float16)
    encT[:, :n] = rng.uniform(-1, 1, (E, n)).astype(np.float16)
    dout = (rng.standard_normal((n, 4)) * 0.05 * dout_scale).astype(np.float16)
    half = _rtz if defect == "rtz" else (lambda a: a.astype(np.float16))
    x = encT[:, :n].astype(np.float32)
    acts = np.zeros((L, W, Sp), np.float16)
    for l in range(L):
        z = mats[l] @ x
        if defect == "short_k" and l == min(1, L - 1):
            rows = [W - 32, W - 31, W - 28, W - 27]          # four features one k-step (16 inputs) short
            z[rows] = mats[l][rows, :-16] @ x[:-16]
        acts[l, :, :n] = half(np.maximum(z, 0))
        x = acts[l, :, :n].astype(np.float32)
    bits = acts.view(np.uint16) != 0
    z = mats[L] @ x
    out = np.ascontiguousarray(half(1 / (1 + np.exp(-z)) if sigmoid else z).T)
    g, y = dout.astype(np.float32).T, out[:, :4].astype(np.float32).T
    dzL = np.zeros((16, Sp), np.float16)
    dzL[:4, :n] = half(g * y * (1 - y) if sigmoid and defect != "no_sigmoid_derivative" else g)
    dz = np.zeros((L, W, Sp), np.float16)

    def mask_of(l):
        return bits[min(l + 1, L - 1) if defect == "mask_next" else l, :, :n]

    dz[L - 1, :, :n] = half(np.where(mask_of(L - 1), mats[L][:4].T @ dzL[:4, :n].astype(np.float32), 0))
    for l in range(L - 1, 0, -1):
        w = mats[l] if defect == "no_transpose" and l == L - 1 else mats[l].T
        dz[l - 1, :, :n] = half(np.where(mask_of(l - 1), w @ dz[l, :, :n].astype(np.float32), 0))
    dencT = np.zeros((E, Sp), np.float16)
    dencT[:, :n] = half(mats[0].T @ dz[0, :, :n].astype(np.float32))
    words = T.pack_masks(bits)
    if defect == "swap_h":
        words = words[:, :, ::-1]
    live = np.ones(Sp // 256, np.uint8)
    if live_list is not None:
        cols = T.compact_columns(live_list)
        k = cols.size
        rest = np.setdiff1d(np.arange(Sp), cols)
        end = -(-k // 256) * 256
        sent = np.uint16(T.SENTINEL)
        cz, czL = np.full((L, W, Sp), sent).view(np.float16), np.full((16, Sp), sent).view(np.float16)
        cz[:, :, :end], czL[:, :end] = 0, 0
        shift = 32 if defect == "shift_slot" else 0
        cz[:, :, shift:k + shift], czL[:, shift:k + shift] = dz[:, :, cols], dzL[:, cols]
        dz, dzL = cz, czL
        acts.view(np.uint16)[:, :, rest] = sent
        words = words.copy()
        words[:, rest] = np.uint64(0x7E5A7E5A7E5A7E5A)
        dencT[:, rest] = 7
        live = np.where(np.arange(Sp // 256) < end // 256, 1, 0x5A).astype(np.uint8)
    raw = T.encode(T.Workspace(acts, dz, dzL, words, live), W, L, Sp)
    return params, encT, out, dout, dencT, raw


def _check(W, L, E, n, sigmoid, **kw):
    report = T.Report()
    params, encT, out, dout, dencT, raw = _standin(W, L, E, n, sigmoid, **kw)
    if kw.get("live_list") is not None:
        T.check_live(report, raw, params, W, L, E, sigmoid, n, kw["live_list"], encT, out, dout, dencT, 7)
    else:
        T.check_saved(report, raw, params, W, L, E, sigmoid, n, encT, out, dout, dencT)
    return report


def _live_list(n, seed=0):
    P = n // 32
    rng = np.random.default_rng(seed)
    live = rng.random(P) < 0.3
    live[[0, P - 1]] = True
    return np.nonzero(live)[0]


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("W,L,E,n", SHAPES)
def test_standin_passes_the_bound_in_every_stage(W, L, E, n, sigmoid, capsys):
    report = _check(W, L, E, n, sigmoid, seed=W + L)
    assert len(report) == 2 * L + 3                        # acts and dz per layer, out, dzL, dencT
    small = _check(W, L, E, n, sigmoid, seed=W + L, dout_scale=2.0 ** -6)     # most of dz[0] subnormal
    report.print(f"stand-in {W}x{L} E{E} n{n} sigmoid={int(sigmoid)}")
    with capsys.disabled():
        print("\n" + report.summary(f"stand-in {W}x{L} E{E} n{n} sigmoid={int(sigmoid)}: largest err / bound (share equal to fp16(ref))"))
        print(small.summary(f"stand-in {W}x{L} E{E} n{n} sigmoid={int(sigmoid)} dout x 2^-6"))
    # a half-ulp bound: the products' stages sit just under it (dzL without the sigmoid is a copy: 0)
    assert max(r for s, r, _ in report if s != "dzL") > 0.9


@pytest.mark.parametrize("W,L,E,n", [(128, 3, 16, 704), (64, 4, 176, 3200)])
def test_standin_passes_in_the_live_list_form(W, L, E, n):
    _check(W, L, E, n, True, seed=3, live_list=_live_list(n))


@pytest.mark.parametrize("W,L,E,n", SHAPES)
def test_subnormal_case_is_mostly_subnormal(W, L, E, n):
    params, encT, out, dout, dencT, raw = _standin(W, L, E, n, True, seed=W + L, dout_scale=2.0 ** -6)
    dz0 = T.decode(raw, W, L, encT.shape[1]).dz[0, :, :n].astype(np.float64)
    nz = dz0[dz0 != 0]
    assert (np.abs(nz) < 2.0 ** -14).mean() > 0.5, float((np.abs(nz) < 2.0 ** -14).mean())


# one k-step short needs 32 inputs; swapping W and W^T needs two hidden layers
DEFECTS = ["short_k", "rtz", "mask_next", "swap_h", "no_transpose", "no_sigmoid_derivative"]


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("W,L,E,n", SHAPES)
def test_negative_controls_fail_the_shared_assertion(W, L, E, n, defect):
    stage = {"short_k": r"acts\[1\]", "rtz": r"acts\[0\]", "mask_next": r"dz\[", "swap_h": r"masks\[0\]", "no_transpose": r"dz\[",
             "no_sigmoid_derivative": "dzL"}[defect]
    with pytest.raises(AssertionError, match=stage):
        _check(W, L, E, n, True, seed=W + L, defect=defect)


@pytest.mark.parametrize("W,L,E,n", [(128, 3, 16, 704), (64, 4, 176, 3200)])
def test_compact_dz_shifted_by_one_slot_fails(W, L, E, n):
    with pytest.raises(AssertionError, match=r"dzL|dz\["):
        _check(W, L, E, n, True, seed=3, live_list=_live_list(n), defect="shift_slot")


@pytest.mark.parametrize("W,L", [(128, 3), (64, 2)])
def test_workspace_image_round_trips(W, L):
    """Random tensors and random mask bits through encode -> decode; single mask bits land where TrainWs and the kernels put
    them: byte h * 8 + kk of a sample's 16, bit j, for feature 16 kk + 8 (j >> 2) + 4 h + (j & 3)."""
    rng = np.random.default_rng(W)
    Sp = 512
    h16 = lambda *s: rng.standard_normal(s).astype(np.float16)
    bits = rng.random((L, W, Sp)) < 0.5
    ws = T.Workspace(h16(L, W, Sp), h16(L, W, Sp), h16(16, Sp), T.pack_masks(bits), rng.integers(0, 2, Sp // 256).astype(np.uint8))
    for lean in (False, True):
        raw = T.encode(ws, W, L, Sp, lean)
        lay = T.layout(W, L, Sp, lean)
        assert raw.size == lay.bytes == ((1 if lean else 2) * L * W * Sp + 16 * Sp) * 2 + L * Sp * 16 + 16
        back = T.decode(raw, W, L, Sp, lean)
        assert (back.acts is None) if lean else np.array_equal(back.acts.view(np.uint16), ws.acts.view(np.uint16))
        for a, b in ((back.dz, ws.dz), (back.dzL, ws.dzL)):
            np.testing.assert_array_equal(a.view(np.uint16), b.view(np.uint16))
        np.testing.assert_array_equal(back.words, ws.words)
        np.testing.assert_array_equal(back.live, ws.live)
        np.testing.assert_array_equal(T.mask_bits(back.words, W), bits)
    lay = T.layout(W, L, Sp)
    for l, s, f in [(0, 0, 0), (L - 1, 300, 5), (1, 17, W - 1), (0, 511, 37), (L - 1, 1, 12)]:
        one = np.zeros((L, W, Sp), bool)
        one[l, f, s] = True
        raw = T.encode(T.Workspace(ws.acts, ws.dz, ws.dzL, T.pack_masks(one), ws.live), W, L, Sp)
        kk, h, j = f // 16, (f >> 2) & 1, (f & 3) + 4 * ((f >> 3) & 1)
        assert T.perm_feature(kk, h, j) == f
        m = raw[lay.masks:lay.live]
        at = (l * Sp + s) * 16 + h * 8 + kk
        assert m[at] == 1 << j and int(m.astype(np.int64).sum()) == 1 << j
    if W == 64:
        assert not (ws.words >> np.uint64(32)).any()


@pytest.mark.parametrize("W,L,E,act,n", [(64, 4, 48, 1, 300), (128, 8, 112, 1, 300), (64, 1, 16, 0, 5), (128, 2, 48, 0, 257)])
def test_free_running_chain_reproduces_the_oracle(oracle, W, L, E, act, n):
    """tests/test_gpu_train.py's bars for the kernels against the oracle, here for the composed restatements: activations 2e-2,
    outputs 1e-2 (sigmoid) / 3e-2 absolute, weight gradients 3e-2 of the largest entry and 2e-2 of the norm, d(encoding) 2e-2
    of its norm -- the backward from the chain's own forward state, as there."""
    rng = np.random.default_rng(W + L + n)
    params = scenes.xavier_params_fp16(W, L, E, seed=W + L + n)
    enc = rng.uniform(-1, 1, (n, E)).astype(np.float16)
    dout = (rng.standard_normal((n, 4)) * 0.05).astype(np.float16)
    acts, out, dparams, denc = T.free_chain(params, W, L, E, bool(act), enc, dout)
    o_acts, o_out = oracle.mlpe_forward(W, L, act, params, enc)
    np.testing.assert_allclose(out.astype(np.float32), o_out.astype(np.float32), rtol=0, atol=1e-2 if act else 3e-2)
    np.testing.assert_allclose(acts.astype(np.float32), o_acts.astype(np.float32), rtol=0, atol=2e-2)
    want_dp, want_denc = oracle.mlpe_backward(W, L, act, params, enc, acts, out, dout)
    scale = np.abs(want_dp).max()
    assert scale > 0
    assert np.abs(dparams - want_dp).max() < 3e-2 * scale
    assert np.linalg.norm(dparams - want_dp) < 2e-2 * np.linalg.norm(want_dp)
    assert np.all(dparams[-16 * W:].reshape(16, W)[4:] == 0)
    assert np.linalg.norm(denc - want_denc) < 2e-2 * np.linalg.norm(want_denc) + 1e-6
