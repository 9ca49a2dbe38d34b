"""Teacher-forced float64 restatements of the training MLP's stages (plain numpy; a helper module, not a conftest).

mlp_train_fwd_kernel and mlp_bwd_kernel leave every stage's result in the training workspace.  Each stage is ONE matrix product
of fp16 operands accumulated in fp32, an elementwise step, and ONE rounding to fp16.  Restated in float64 from the kernel's OWN
stored inputs of that stage (not from a free-running chain, which drifts from an fp16 chain layer by layer), the only
differences left are that fp32 accumulation and that fp16 rounding, so the distance has a derived bound:

    u = 2^-24 (fp32 unit roundoff), K = contraction length, mag = the same product over absolute values
    bound = 2^-11 |ref| (1 + 2^-10)  +  2^-25  +  K u mag
            half an fp16 ulp            half the fp16 subnormal spacing      the fp32 accumulation, as _k_wgrad of
                                                                             tests/test_gpu_deterministic_gradients.py counts it
    (the factor 1 + 2^-10 lets the half ulp be taken at the fp32 value instead of at ref).

Nothing flushes on the way: subnormal fp16 operands enter the products with their value, and a result below
2^-14 is stored as the nearest subnormal -- the 2^-25 term is that rounding.

dZ_L = g y (1 - y) is three fp32 roundings of one term (g y, 1 - y, their product) and the one to fp16: the accumulation term
is 3 u |ref|; without the sigmoid the fp16 gradient is copied.

The sigmoid output y = sigmoidf_fast(z) = v_rcp_f32(1 + v_exp_f32(-z log2e)) (mlp_internal.h:43), z the fp32 accumulator:
  * z carries K u mag_z, which reaches y through y' = y (1 - y);
  * m = fl(-z * fl(log2 e)) has two relative roundings (the constant's and the product's): |dm| <= 2 u |z| log2 e, and
    2^m = e^(m ln 2), so the exponential e carries 2 u |z| relative from its argument and 1 ulp = 2 u from v_exp_f32;
    d(1 / (1 + e)) / y = -(1 - y) de / e, so this arrives at y scaled by (1 - y): (1 - y) (2 |z| + 2) u;
  * the sum 1 + e is one fp32 rounding (u) and v_rcp_f32 is 1 ulp (2 u): 3 u relative on y;
  bound_y = 2^-11 y (1 + 2^-10) + 2^-25 + (1 + 2^-10) y [(1 - y) (K u mag_z + (2 |z| + 2) u) + 3 u].
No constant here comes from running a kernel.

Workspace layout (TrainWs in rtx_nerf_amd/csrc/train.hip), bytes from the base, Sp = samples padded to 256:
    [acts fp16 [L][W][Sp] |] dz fp16 [L][W][Sp] | dzL fp16 [16][Sp] | masks u64 [L][Sp][2] | one live flag per 256-sample tile,
    padded to 16 B;   the lean layout has no acts.
Word h of a sample's mask pair holds at bit 8 kk + j the feature perm_feature(kk, h, j) (W / 16 k-steps: 64 bits at W = 128, the
low 32 at W = 64).  Tensors here are feature-major ([features][samples]) like the kernel's; `out` and `dout` are [samples][16 | 4].
"""
from collections import namedtuple

import numpy as np

from _mlp_float64 import layers_of

U = 2.0 ** -24
SENTINEL = 0x7E5A            # an fp16 NaN bit pattern (bytes 5A 7E): what the tests pre-fill a workspace with

Layout = namedtuple("Layout", "acts dz dzL masks live bytes")
Workspace = namedtuple("Workspace", "acts dz dzL words live")     # acts: None when lean; words: u64 [L][Sp][2]; live: u8 [Sp / 256]


def perm_feature(kk, h, j):
    """Feature held by element j of lane-half h in k-step kk (restated from mlp_internal.h, deliberately not imported)."""
    return 16 * kk + 8 * (j >> 2) + 4 * h + (j & 3)


# ------------------------------------------------------------------------------------------------------- workspace
def layout(W, L, Sp, lean=False):
    assert Sp % 256 == 0
    dz = 0 if lean else L * W * Sp * 2
    dzL = dz + L * W * Sp * 2
    masks = dzL + 16 * Sp * 2
    live = masks + L * Sp * 16
    return Layout(0, dz, dzL, masks, live, live + (Sp // 256 + 15) // 16 * 16)


def decode(raw, W, L, Sp, lean=False):
    """raw: the workspace's bytes (uint8, at least layout().bytes of them) -> Workspace of copies."""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    lay = layout(W, L, Sp, lean)
    assert raw.size >= lay.bytes, (raw.size, lay.bytes)

    def halves(off, *shape):
        return raw[off:off + 2 * int(np.prod(shape))].copy().view(np.float16).reshape(shape)

    acts = None if lean else halves(lay.acts, L, W, Sp)
    words = raw[lay.masks:lay.live].copy().view("<u8").reshape(L, Sp, 2)
    return Workspace(acts, halves(lay.dz, L, W, Sp), halves(lay.dzL, 16, Sp), words, raw[lay.live:lay.live + Sp // 256].copy())


def encode(ws, W, L, Sp, lean=False, fill=0):
    """The inverse of decode: a byte image of the workspace."""
    lay = layout(W, L, Sp, lean)
    raw = np.full(lay.bytes, fill, np.uint8)
    if not lean:
        raw[lay.acts:lay.dz] = np.ascontiguousarray(ws.acts, np.float16).reshape(-1).view(np.uint8)
    raw[lay.dz:lay.dzL] = np.ascontiguousarray(ws.dz, np.float16).reshape(-1).view(np.uint8)
    raw[lay.dzL:lay.masks] = np.ascontiguousarray(ws.dzL, np.float16).reshape(-1).view(np.uint8)
    raw[lay.masks:lay.live] = np.ascontiguousarray(ws.words, "<u8").reshape(-1).view(np.uint8)
    raw[lay.live:lay.live + Sp // 256] = ws.live
    return raw


def mask_bits(words, W):
    """u64 [L][S][2] -> bool [L][W][S]"""
    L, S, _ = words.shape
    out = np.zeros((L, W, S), bool)
    for kk in range(W // 16):
        for h in range(2):
            for j in range(8):
                out[:, perm_feature(kk, h, j), :] = (words[:, :, h] >> np.uint64(8 * kk + j)) & np.uint64(1)
    return out


def pack_masks(bits):
    """bool [L][W][S] -> u64 [L][S][2]"""
    L, W, S = bits.shape
    words = np.zeros((L, S, 2), np.uint64)
    for kk in range(W // 16):
        for h in range(2):
            for j in range(8):
                words[:, :, h] |= bits[:, perm_feature(kk, h, j), :].astype(np.uint64) << np.uint64(8 * kk + j)
    return words


def is_sentinel(a):
    """Elementwise: an fp16 array still holds the pre-fill pattern."""
    return np.ascontiguousarray(a).view(np.uint16) == SENTINEL


def compact_columns(live_list):
    """In-place column of every compact column slot * 32 + sample of a live list (mlp_bwd_kernel with a list writes dz / dzL
    compactly, in list order)."""
    return (np.asarray(live_list, np.int64)[:, None] * 32 + np.arange(32)[None, :]).reshape(-1)


# ------------------------------------------------------------------------------------------------------- one stage each
def _f64(a):
    return np.asarray(a).astype(np.float64)


def hidden_forward(w, x):
    """max(W X, 0): w [out][in], x fp16 [in][n] (X_{-1} = encT)."""
    w, x = _f64(w), _f64(x)
    return np.maximum(w @ x, 0.0), np.abs(w) @ np.abs(x)


def output_layer(w, x, sigmoid):
    """16 rows.  Returns (y, mag_z, z): y = z or 1 / (1 + exp(-z))."""
    w, x = _f64(w), _f64(x)
    z = w @ x
    with np.errstate(over="ignore"):
        y = 1.0 / (1.0 + np.exp(-z)) if sigmoid else z
    return y, np.abs(w) @ np.abs(x), z


def dz_out(out, dout, sigmoid):
    """[16][n] from the STORED fp16 out [n][16] and dout [n][4]: rows 0..3 g y (1 - y) or g, rows 4..15 zero."""
    g, y = _f64(dout).T, _f64(out)[:, :4].T
    ref = np.zeros((16, g.shape[1]))
    ref[:4] = g * y * (1.0 - y) if sigmoid else g
    return ref, np.abs(ref)


def chain_step(w, dz_next, mask):
    """mask (*) (W^T dZ): w [out][in] of the layer dZ belongs to, dz_next fp16 [out][n], mask bool [in][n]."""
    w, d = _f64(w), _f64(dz_next)
    return np.where(mask, w.T @ d, 0.0), np.where(mask, np.abs(w).T @ np.abs(d), 0.0)


def last_hidden_dz(w_out, dzL, mask):
    """dz[L-1] from dzL and the output layer's first 4 rows (dzL's other rows are zero), as the kernel has it: one 16-row
    k-step, so the bound takes K = 16."""
    return chain_step(_f64(w_out)[:4], _f64(dzL)[:4], mask)


def denc(w0, dz0):
    """dencT = W_0^T dz[0]"""
    w, d = _f64(w0), _f64(dz0)
    return w.T @ d, np.abs(w).T @ np.abs(d)


# ------------------------------------------------------------------------------------------------------- the bounds
def bound_fp16(ref, mag, K):
    return 2.0 ** -11 * np.abs(ref) * (1 + 2.0 ** -10) + 2.0 ** -25 + K * U * mag


def bound_dz_out(ref, sigmoid):
    return bound_fp16(ref, np.abs(ref), 3 if sigmoid else 0)


def bound_output(y, mag_z, z, K, sigmoid):
    if not sigmoid:
        return bound_fp16(y, mag_z, K)
    return (2.0 ** -11 * y * (1 + 2.0 ** -10) + 2.0 ** -25
            + (1 + 2.0 ** -10) * y * ((1.0 - y) * (K * U * mag_z + (2 * np.abs(z) + 2) * U) + 3 * U))


# ------------------------------------------------------------------------------------------------------- the shared assertion
class Report(list):
    """(stage, largest err / bound, share of values equal to fp16(ref)) per checked stage; printed, never asserted on."""

    def lines(self, title=""):
        return [f"measured {title} {s}: err / bound {r:.3f}, equal to fp16(ref) {e:.4f}" for s, r, e in self]

    def summary(self, title=""):
        """One line: per kind of stage (acts, out, dzL, dz, dencT) the largest err / bound and the smallest exact share."""
        kinds = {}
        for s, r, e in self:
            k = s.split("[")[0]
            a, b = kinds.get(k, (0.0, 1.0))
            kinds[k] = (max(a, r), min(b, e))
        return f"measured {title}: " + ", ".join(f"{k} {r:.3f} ({e:.4f})" for k, (r, e) in kinds.items())

    def print(self, title=""):
        for line in self.lines(title):
            print(line)


def check_stage(report, stage, got, ref, bound):
    """THE assertion: every element of `got` (fp16) is finite and within `bound` of `ref`.  No element is excluded."""
    got = np.asarray(got)
    assert got.dtype == np.float16 and got.shape == ref.shape == bound.shape, (stage, got.dtype, got.shape, ref.shape)
    g = got.astype(np.float64)
    finite = np.isfinite(g)
    err = np.where(finite, np.abs(g - ref), np.inf)
    ratio = err / bound
    with np.errstate(over="ignore"):
        exact = float((got == ref.astype(np.float16)).mean()) if got.size else 1.0
    worst = float(ratio.max()) if got.size else 0.0
    if report is not None:
        report.append((stage, worst, exact))
    bad = err > bound
    assert not bad.any(), (f"{stage}: {int(bad.sum())} of {bad.size} elements outside the bound ({int((~finite).sum())} not finite), "
                           f"largest err / bound {worst:.3g} at {np.unravel_index(int(np.argmax(ratio)), ratio.shape)}")


def check_forward(report, params, W, L, E, sigmoid, encT, acts, bits, out):
    """encT fp16 [E][n], acts fp16 [L][W][n], bits bool [L][W][n] (decoded masks), out fp16 [n][16] or None (the live pass
    stores none): every layer from the kernel's own stored input of that layer; mask bit == (stored activation != +0)."""
    mats = layers_of(params, W, L, E)
    x = encT
    for l in range(L):
        ref, mag = hidden_forward(mats[l], x)
        check_stage(report, f"acts[{l}]", acts[l], ref, bound_fp16(ref, mag, x.shape[0]))
        stored_nonzero = np.ascontiguousarray(acts[l]).view(np.uint16) != 0
        wrong = bits[l] != stored_nonzero
        assert not wrong.any(), f"masks[{l}]: {int(wrong.sum())} bits differ from (stored activation != +0), first at {np.argwhere(wrong)[0]}"
        x = acts[l]
    if out is not None:
        y, mag, z = output_layer(mats[L], x, sigmoid)
        check_stage(report, "out", np.ascontiguousarray(out.T), y, bound_output(y, mag, z, W, sigmoid))


def check_backward(report, params, W, L, E, sigmoid, out, dout, bits, dzL, dz, dencT, dz_last=None):
    """out fp16 [n][16], dout fp16 [n][4], bits bool [L][W][n], dzL fp16 [16][n], dz fp16 [L][W][n], dencT fp16 [E][n] or None.
    dz_last: dz[L-1] where the workspace does not hold it (skip_last_dz); dz[L-1] itself is then not checked."""
    mats = layers_of(params, W, L, E)
    ref, _ = dz_out(out, dout, sigmoid)
    check_stage(report, "dzL", dzL, ref, bound_dz_out(ref, sigmoid))
    if dz_last is None:
        ref, mag = last_hidden_dz(mats[L], dzL, bits[L - 1])
        check_stage(report, f"dz[{L - 1}]", dz[L - 1], ref, bound_fp16(ref, mag, 16))
    nxt = dz[L - 1] if dz_last is None else dz_last
    for l in range(L - 1, 0, -1):
        ref, mag = chain_step(mats[l], nxt, bits[l - 1])
        check_stage(report, f"dz[{l - 1}]", dz[l - 1], ref, bound_fp16(ref, mag, W))
        nxt = dz[l - 1]
    if dencT is not None:
        ref, mag = denc(mats[0], nxt)
        check_stage(report, "dencT", dencT, ref, bound_fp16(ref, mag, W))


# ------------------------------------------------------------------------------------------------------- whole workspaces
def _zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint16).any()


def check_saved(report, raw, params, W, L, E, sigmoid, n, encT, out, dout, dencT, lean=False, dz_last=None, skip_last_dz=False):
    """A list-free run (train_forward[_lean] + train_backward[_lean]) over a workspace pre-filled with SENTINEL.
    raw: the workspace's bytes; encT fp16 [E][Sp] with zero padding columns; out fp16 [n][16]; dout fp16 [n][4]; dencT fp16
    [E][Sp] or None.  Every element with sample < n goes through check_stage; padding is what the kernels define:
      forward   acts past n are +0; the masks past n are those of the padding columns' input (zero encT -> zero words);
      backward  a 256-sample tile whose dZ_L is zero everywhere has live flag 0, keeps the pre-fill in dz / dzL and has zero
                dencT columns; in every other tile the columns past n are zero in dz, dzL and dencT.
    Returns the decoded Workspace."""
    Sp = encT.shape[1]
    assert Sp == -(-n // 256) * 256
    ws = decode(raw, W, L, Sp, lean)
    bits = mask_bits(ws.words, W)
    if W == 64:
        assert not (ws.words >> np.uint64(32)).any(), "W = 64: a mask word uses its low 32 bits only"
    assert not ws.words[:, n:].any(), "mask words of the padding columns"
    if not lean:
        check_forward(report, params, W, L, E, sigmoid, encT[:, :n], ws.acts[:, :, :n], bits[:, :, :n], out)
        assert _zero_bits(ws.acts[:, :, n:]), "acts past n are +0"
    if dout is None:
        return ws
    flags = ws.live
    assert set(np.unique(flags)) <= {0, 1}, flags
    col_live = np.repeat(flags.astype(bool), 256)
    c = np.nonzero(col_live[:n])[0]
    dead = np.nonzero(~col_live[:n])[0]
    stored = slice(0, L - 1 if skip_last_dz else L)
    check_backward(report, params, W, L, E, sigmoid, out[c], dout[c], bits[:, :, c], ws.dzL[:, c], ws.dz[:, :, c],
                   None if dencT is None else dencT[:, c], dz_last=None if dz_last is None else dz_last[:, c])
    pad_live = np.nonzero(col_live[n:])[0] + n
    assert not ws.dzL[:, pad_live].astype(np.float32).any() and not ws.dz[stored][:, :, pad_live].astype(np.float32).any(), "dz / dzL past n"
    if skip_last_dz:
        assert is_sentinel(ws.dz[L - 1]).all(), "skip_last_dz: dz[L-1] is not stored"
    # dead tiles: nothing the chain would have produced there differs from zero by more than its rounding
    ref, _ = dz_out(out[dead], dout[dead], sigmoid)
    assert np.all(np.abs(ref) <= bound_dz_out(ref, sigmoid)), "a tile flagged dead has a non-zero dZ_L"
    dead_cols = np.nonzero(~col_live)[0]
    assert is_sentinel(ws.dzL[:, dead_cols]).all() and is_sentinel(ws.dz[:, :, dead_cols]).all(), "a dead tile's dz / dzL were written"
    if dencT is not None:
        assert not dencT[:, dead_cols].astype(np.float32).any(), "a dead tile's dencT columns are zero"
        assert not dencT[:, n:].astype(np.float32).any(), "dencT past n"
    return ws


def check_live(report, raw, params, W, L, E, sigmoid, n, live_list, encT, out, dout, dencT, fill):
    """The live-list forms (train_forward_live + train_backward_live) over a workspace pre-filled with SENTINEL; n whole
    32-sample segments.  Listed segments: acts and masks in place and within the bound, dencT in place; dz / dzL compact at
    slot * 32 + sample, restated from the compact tensors (masks, out and dout gathered in list order).  Everything else keeps
    what it held: SENTINEL in the workspace, `fill` in dencT.  Slots past the list in the last block of eight are zero."""
    Sp = encT.shape[1]
    assert n % 32 == 0 and Sp == -(-n // 256) * 256
    ws = decode(raw, W, L, Sp)
    bits = mask_bits(ws.words, W)
    cols = compact_columns(live_list)
    rest = np.setdiff1d(np.arange(Sp), cols)
    k = cols.size
    check_forward(report, params, W, L, E, sigmoid, encT[:, cols], ws.acts[:, :, cols], bits[:, :, cols], None)
    assert is_sentinel(ws.acts[:, :, rest]).all(), "acts outside the listed segments"
    assert (ws.words[:, rest].view(np.uint16) == SENTINEL).all(), "masks outside the listed segments"
    if dout is None:
        return ws
    check_backward(report, params, W, L, E, sigmoid, out[cols], dout[cols], bits[:, :, cols], ws.dzL[:, :k], ws.dz[:, :, :k],
                   None if dencT is None else dencT[:, cols])
    end = -(-k // 256) * 256
    assert not ws.dzL[:, k:end].astype(np.float32).any() and not ws.dz[:, :, k:end].astype(np.float32).any(), "slots past the list"
    assert is_sentinel(ws.dzL[:, end:]).all() and is_sentinel(ws.dz[:, :, end:]).all(), "dz / dzL past the list's last block"
    assert np.all(ws.live[:end // 256] == 1)
    if dencT is not None:
        assert np.all(dencT[:, rest] == np.float16(fill)), "dencT outside the listed segments"
    return ws


# ------------------------------------------------------------------------------------------------------- the free-running chain
def free_chain(params, W, L, E, sigmoid, enc, dout):
    """The whole forward and backward in float64 with fp16 (round-to-nearest) storage between the stages, each stage fed the
    previous one's OWN result: what the one-stage restatements compose to.  enc fp16 [n][E], dout fp16 [n][4].
    Returns acts fp16 [L][n][W] and out fp16 [n][16] (the oracle's layouts), dparams float64 (tcnn layout), denc float64 [n][E]."""
    mats = layers_of(params, W, L, E)
    xs = [np.ascontiguousarray(np.asarray(enc, np.float16).T)]
    for l in range(L):
        xs.append(hidden_forward(mats[l], xs[-1])[0].astype(np.float16))
    out = np.ascontiguousarray(output_layer(mats[L], xs[-1], sigmoid)[0].astype(np.float16).T)
    dzL = dz_out(out, dout, sigmoid)[0].astype(np.float16)
    dzs = [None] * L
    dzs[L - 1] = last_hidden_dz(mats[L], dzL, xs[L] != 0)[0].astype(np.float16)
    for l in range(L - 1, 0, -1):
        dzs[l - 1] = chain_step(mats[l], dzs[l], xs[l] != 0)[0].astype(np.float16)
    grads = [_f64(d) @ _f64(x).T for d, x in zip(dzs + [dzL], xs)]
    acts = np.stack([np.ascontiguousarray(x.T) for x in xs[1:]])
    return acts, out, np.concatenate([g.reshape(-1) for g in grads]), denc(mats[0], dzs[0])[0].T
