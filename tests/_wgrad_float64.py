"""Float64 restatement of the RECOMPUTING weight-gradient kernels, element by element (a helper module, not a conftest; numpy
here, torch only through the tensors a caller hands in).

mlp_bwd_fused64_kernel<L, KS0> (64-wide models) and wgrad_recompute_kernel / wgrad_recompute_all_kernel (the 8 x 128 lean path)
never store the activations: they rebuild them on the chip and accumulate dW_l = dZ_l X_l^T in registers.  They claim to rebuild
the SAME fp16 values the saved-activation path stores, so the reference is built from that path's workspace on the same inputs
(acts | dz | dzL, X_0 = encT; layout of tests/_train_float64.py, whose tests hold those tensors to float64):

    ref_l = dZ_l X_l^T      mag_l = |dZ_l| |X_l|^T      in float64, concatenated in tcnn order, the 16 x W output layer included.

The claim is a PRECONDITION the GPU tests assert, not assume: the fused kernel's dencT equals the saved chain's bit for bit (dencT =
W_0^T dZ_0 hangs on every recomputed activation through the masks of the whole chain), the lean path's masks, dz and dzL equal
the saved path's bit for bit.  With it, all that is left between kernel and reference is the fp32 summation:

    bound = u |ref| + k u mag,     u = 2^-24,     no flat tolerance anywhere

k is derived from the kernels, as _k_wgrad of tests/test_gpu_deterministic_gradients.py is for the saved path (an addition on
the path of a term costs at most u times the sum of the magnitudes):
  * a block keeps its sums in fp32 registers over ALL its tiles (persistent loop: tiles b, b + grid, ...), so a term sits under
    every addition of every tile of its block: ceil(n_tiles / grid) tiles;
  * a tile is 256 samples = 16 MFMA k-steps of 16 samples (v_mfma_f32_32x32x16_f16: 4 images x 4 k-steps in the fused kernel, two
    halves of 8 in the lean one): at most 16 additions inside the instruction a term enters through and 16 accumulations of one
    instruction's result onto the running sum -- at most 32 dependent additions per tile;
  * then ONE atomic per block and element -- at most `grid` partials meet in any order (fp32 atomics), or exactly (the
    deterministic mode's fixed point, which is no worse) -- and the fold / the final rounding: + 2.
        k_recompute(n_tiles, grid) = 32 ceil(n_tiles / grid) + grid + 2
  * grid, from the launchers (train.hip): min(n_tiles, CUs) for mlp_bwd_fused64_kernel and for each per-pass
    wgrad_recompute_kernel.  wgrad_recompute_all_kernel (n_tiles >= 4 CUs) deals CUs / 8 slots per XCD to its three passes,
    split[0] : split[1] - split[0] : rest of 32 (9 : 11 : 12 reading encT, 8 : 11 : 13 encoding for itself); a pass runs on its
    share of the blocks only.  all_pass_grid() returns the SMALLEST share: its blocks run the most tiles each, which is what k
    grows with, so that k covers all three passes (a larger share g' > g trades 32 n_tiles (1 / g - 1 / g') tile additions for
    g' - g atomics: fewer in all wherever 32 n_tiles >= g g', and here n_tiles >= 4 CUs with g, g' < CUs / 2).
  * with a live list a tile is any eight listed segments: n_tiles = ceil(listed / 8).  Tiles the chain flagged dead are stepped
    over and only shorten a block's sum.
  One place sums differently and is held to the same k all the same: the lean output layer's 16 x 128 gradient is kept per WAVE
  for the wave's own 64 samples of a tile (4 k-steps) and every wave adds its share -- 4 atomics per block and element, path
  16 + 4 ceil(n_tiles / grid) + 4 grid + 2.  That is below k for a handful of blocks and above it for whole-chip grids (1054
  against 354 at 256 CUs and three tiles per block); the tests keep k, the tighter of the two, for every layer.
The deterministic mode adds one term, and only there.  Its partials do not meet as floats: grad_add rounds each to the fixed
point's grid, __float2ll_rn(v 2^40), an ABSOLUTE error of up to 2^-41 per atomic whatever the size of the sum, before the exact
integer sum and the fold's single rounding.  For gradients near 2^-40 k u mag is smaller than that (first seen on the MI355X at
64x4, E = 64, n = 5, one block: an element of layer 0 at 1.45 of the bound without the term, 0.04 in the default mode), so
    bound_det = bound + atomics 2^-41,     atomics = the partials per element: grid (4 grid for the lean output layer; for the
                                            single launch the whole launch's blocks, which no pass share exceeds)
as the scatter's bound of tests/test_gpu_deterministic_gradients.py counts its own (n_contrib 2^-41).  The default mode's bound
has no absolute term.
No constant here comes from running a kernel.  The CU count is the device's (multi_processor_count), never a literal.

emulate() restates the block-wise fp32 accumulation in numpy (grid, tiles per block, 16-sample k-steps); with it
tests/test_wgrad_float64_reference.py shows, on the CPU, that a faithful kernel stays inside the bound and what falls outside it.
"""
from collections import namedtuple

import numpy as np

from _train_float64 import U, layout   # noqa: F401  (layout: where the workspace keeps the tensors the reference is read from)

TILE = 256          # samples per block tile (kTile)
KSTEP = 16          # samples per MFMA k-step


def layer_sizes(W, L, E):
    """(rows, columns) per layer in tcnn order"""
    return [(W, E)] + [(W, W)] * (L - 1) + [(16, W)]


def _cat(parts):
    if isinstance(parts[0], np.ndarray):
        return np.concatenate(parts)
    import torch
    return torch.cat(parts)


def _f64(a):
    return a.astype(np.float64) if isinstance(a, np.ndarray) else a.double()


def reference(dZ, X):
    """dZ, X: per layer [rows][n] and [columns][n] (fp16 values; numpy arrays or torch tensors, on whatever device they live).
    Returns float64 (ref, mag): dZ_l X_l^T and |dZ_l| |X_l|^T, flattened and concatenated in tcnn order."""
    assert len(dZ) == len(X)
    ref, mag = [], []
    for d, x in zip(dZ, X):
        d, x = _f64(d), _f64(x)
        ref.append((d @ x.T).reshape(-1))
        mag.append((abs(d) @ abs(x).T).reshape(-1))
    return _cat(ref), _cat(mag)


# ------------------------------------------------------------------------------------------------------- k and the grids
def n_tiles_of(n, listed=None):
    """256-sample tiles of n samples; with a live list of `listed` segments a tile is eight of them."""
    return -(-listed // 8) if listed is not None else -(-n // TILE)


def persistent_grid(n_tiles, n_cu):
    """mlp_bwd_fused64_kernel and wgrad_recompute_kernel: one block per CU, no more than there are tiles"""
    return max(1, min(n_tiles, n_cu))


def all_pass_used(n_tiles, n_cu, encoding_folded):
    """The launcher's own rule for the single launch (train_backward_lean_impl, default split)"""
    s = (8, 19) if encoding_folded else (9, 20)
    return 0 < s[0] < s[1] < n_cu // 8 and n_tiles >= 4 * n_cu


def all_pass_grid(n_cu, encoding_folded):
    """Blocks of the smallest pass share of wgrad_recompute_all_kernel"""
    slots = n_cu // 8
    s = (8, 19) if encoding_folded else (9, 20)
    s1, s2 = s[0] * slots // 32, s[1] * slots // 32
    return 8 * min(s1, s2 - s1, slots - s2)


def k_recompute(n_tiles, grid):
    return 32 * -(-n_tiles // grid) + grid + 2


FIXED_POINT_HALF = 2.0 ** -41          # half the spacing of the deterministic mode's fixed point (kDetScale = 2^40)


def bound_of(ref, mag, k):
    return U * np.abs(ref) + k * U * mag


def lean_atomics(grid, L):
    """Partials per element and layer of the lean kernels: one per block, four (one per wave) for the output layer"""
    return [grid] * L + [4 * grid]


# ------------------------------------------------------------------------------------------------------- the checker
Result = namedtuple("Result", "bad worst half first")   # bad: elements not inside the bound; per layer: largest err / bound, share above 0.5


def check(got, ref, mag, k, sizes, pre=None, grid=0, det_atomics=None):
    """got: what the kernel left in dparams (fp32); ref, mag: reference(); sizes: layer_sizes().
    pre: what dparams held before the call (default mode's accumulate semantics): got - pre is held to
    bound + grid u (|pre| + |ref|) -- every one of up to `grid` atomics rounds a running sum no larger than |pre| + |ref| + bound.
    grid is the number of atomics per element: one number, or one per layer (lean_atomics: the lean output layer's four per
    block; held to `grid` alone, an element of it came out at 1.02 on the MI355X with three blocks, every other layer at 0.67 to 0.93).
    det_atomics: deterministic mode only -- the partials per element (one number, or one per layer), each rounded to the fixed
    point: + det_atomics 2^-41.
    Counts the elements NOT inside the bound, so a NaN or an Inf counts like any other wrong value; no element is left out."""
    got = np.asarray(got)
    assert got.dtype == np.float32, got.dtype
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert got.shape == ref.shape == mag.shape == (sum(r * c for r, c in sizes),), (got.shape, ref.shape, mag.shape)
    def per_element(a):
        per_layer = [a] * len(sizes) if np.isscalar(a) else list(a)
        assert len(per_layer) == len(sizes)
        return np.concatenate([np.full(r * c, float(v)) for (r, c), v in zip(sizes, per_layer)])

    bound = bound_of(ref, mag, k)
    if det_atomics is not None:
        bound = bound + FIXED_POINT_HALF * per_element(det_atomics)
    with np.errstate(invalid="ignore", over="ignore"):
        val = got.astype(np.float64)
        if pre is not None:
            p = np.asarray(pre).astype(np.float64)
            val = val - p
            bound = bound + per_element(grid) * U * (np.abs(p) + np.abs(ref))
        err = np.abs(val - ref)
        inside = err <= bound                                   # False for NaN
        err = np.where(np.isfinite(err), err, np.inf)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    worst, half, off = [], [], 0
    for r, c in sizes:
        q = ratio[off:off + r * c]
        worst.append(float(q.max()))
        half.append(float((q > 0.5).mean()))
        off += r * c
    bad = int((~inside).sum())
    return Result(bad, worst, half, int(np.argmax(~inside)) if bad else -1)


def lines(title, res):
    """One line per case for the log and the record: largest err / bound per layer, and the share of elements above half of it"""
    return (f"measured {title}: err / bound " + " ".join(f"{w:.3f}" for w in res.worst)
            + f" | largest {max(res.worst):.3f}, share above 0.5: {max(res.half):.5f}, outside: {res.bad}")


# ------------------------------------------------------------------------------------------------------- the emulation
def block_schedule(n_tiles, grid, tiles_per_block=None):
    """Tiles of every block of the persistent loop: b, b + grid, ..."""
    t = -(-n_tiles // grid)
    if tiles_per_block is not None:
        assert tiles_per_block >= t, "tiles left over"
    return [list(range(b, n_tiles, grid)) for b in range(grid)]


def emulate(dZ, X, grid, tiles_per_block=None, ksteps=TILE // KSTEP, schedule=None, pre=None, deterministic=False, live_list=None):
    """One layer, fp32 as the kernels sum it.  dZ fp16 [M][n], X fp16 [N][n]; a tile is `ksteps` k-steps of 16 samples.
    Block b sums its tiles (schedule[b]; default block_schedule) k-step by k-step onto ONE fp32 accumulator; then the blocks'
    partials are added one after the other to `pre` (zeros by default) in fp32 -- or, deterministic, each rounded to the fixed
    point (value x 2^40, round to nearest), summed exactly, rounded once to fp32 and added to `pre`.  live_list: segment indices (32 samples each); the tiles are then made of the listed segments, eight at a time, the
    slots past the list adding zeros.  Returns fp32 [M][N]."""
    dZ, X = np.asarray(dZ, np.float16), np.asarray(X, np.float16)
    n = dZ.shape[1]
    if live_list is not None:
        assert ksteps * KSTEP == TILE
        cols = (np.asarray(live_list, np.int64)[:, None] * 32 + np.arange(32)[None, :]).reshape(-1)
        dZ, X = dZ[:, cols], X[:, cols]
        n = cols.size
    tile = ksteps * KSTEP
    n_tiles = -(-n // tile)
    pad = n_tiles * tile - n
    d32 = np.pad(dZ.astype(np.float32), ((0, 0), (0, pad)))
    x32 = np.pad(X.astype(np.float32), ((0, 0), (0, pad)))
    if schedule is None:
        schedule = block_schedule(n_tiles, grid, tiles_per_block)
    partials = []
    for tiles in schedule:
        if not tiles:
            continue
        acc = np.zeros((dZ.shape[0], X.shape[0]), np.float32)
        for t in tiles:
            for ks in range(ksteps):
                c = slice(t * tile + ks * KSTEP, t * tile + (ks + 1) * KSTEP)
                acc = acc + d32[:, c] @ x32[:, c].T              # fp32 product sum of one instruction, then one fp32 addition
        partials.append(acc)
    base = np.zeros((dZ.shape[0], X.shape[0]), np.float32) if pre is None else np.asarray(pre, np.float32).reshape(dZ.shape[0], X.shape[0])
    if deterministic:
        q = np.sum([np.rint(p.astype(np.float64) * 2.0 ** 40) for p in partials], axis=0)        # exact: |q| < 2^53 at these sizes
        return base + (q * 2.0 ** -40).astype(np.float32)
    total = base.copy()
    for p in partials:
        total = total + p
    return total


def emulate_layers(dZ, X, grid, **kw):
    """emulate() per layer, flattened and concatenated in tcnn order; pre (flat) is split per layer"""
    pre = kw.pop("pre", None)
    out, off = [], 0
    for d, x in zip(dZ, X):
        size = d.shape[0] * x.shape[0]
        out.append(emulate(d, x, grid, pre=None if pre is None else pre[off:off + size], **kw).reshape(-1))
        off += size
    return np.concatenate(out)
