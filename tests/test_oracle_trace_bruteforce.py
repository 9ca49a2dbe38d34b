"""An independent check of the oracle's flat DDA walk (oracle.trace, mode 1), which the GPU traversal is held to bit for
bit: a float64 brute force that shares nothing with it.  For every ray, EVERY cell of a small grid is slab-tested in
float64; the occupied cells with a positive chord, ordered by entry t, must be the walk's segments.

Family: origins outside the grid at radius 2.8..4 (so every ray parameter inside the grid is >= 2.8 - sqrt(3) > 1), aimed
at points inside it, every |d[a]| >= 0.1.  Rounding of the float32 walk under those conditions, eps = 2^-23:
  plane coordinate -1 + i*L (L = fl(2/R), one product, one sum, all values <= 2)            <= 2 eps
  plane - o (|result| < 8)                                                                   <= 2 eps
  so the numerator is off by <= 4 eps, and times 1/d[a] (|1/d| <= 10)                        <= 40 eps
  1/d[a] and the product, half an ulp each, relative to t                                    <= eps * t
  => |t32 - t64| <= 40 eps + eps t <= 41 eps t   (t >= 1)
A chord is the difference of two such values, so a cell whose float64 chord is below 2 * 41 eps t can legitimately be
present in one walk and absent in the other.  The threshold is 128 eps t (82 rounded up to the next power of two), with
t the float64 exit parameter of that cell; cells below it are left out on both sides, and their share is asserted to be
at most 1 %.  The lattice families are not part of this check: there ties are the point, and only bit parity with
the flat walk means anything.
"""
import numpy as np
import pytest

from tools import _trace_cases as TC

EPS = 2.0 ** -23
CHORD_MULTIPLE = 128       # cells with chord64 < CHORD_MULTIPLE * EPS * t_exit are left out on both sides
T_MULTIPLE = 41            # |t32 - t64| <= T_MULTIPLE * EPS * t (derivation above)


def _family(R, n, seed):
    rng = np.random.default_rng([seed, R])
    o = np.zeros((0, 3), np.float32)
    d = np.zeros((0, 3), np.float32)
    while o.shape[0] < n:
        v = rng.standard_normal((4 * n, 3))
        oo = (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2.8, 4.0, (4 * n, 1))).astype(np.float32)
        dd = TC._unit(rng.uniform(-0.95, 0.95, (4 * n, 3)).astype(np.float32) - oo)
        ok = (np.abs(dd) >= 0.1).all(axis=1)
        o, d = np.concatenate([o, oo[ok]]), np.concatenate([d, dd[ok]])
    return np.ascontiguousarray(o[:n]), np.ascontiguousarray(d[:n])


def _brute_force(o, d, R, dense):
    """float64 slab test of every cell against every ray -> t_in, t_out [n, R, R, R] (t_in clipped at 0)."""
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    planes = -1.0 + np.arange(R + 1, dtype=np.float64) * (2.0 / R)
    tn, tf = [], []
    for a in range(3):
        t = (planes[None, :] - o64[:, a:a + 1]) / d64[:, a:a + 1]                   # [n, R+1]
        tn.append(np.minimum(t[:, :-1], t[:, 1:]))
        tf.append(np.maximum(t[:, :-1], t[:, 1:]))
    t_in = np.maximum(np.maximum(tn[0][:, :, None, None], tn[1][:, None, :, None]), tn[2][:, None, None, :])
    t_out = np.minimum(np.minimum(tf[0][:, :, None, None], tf[1][:, None, :, None]), tf[2][:, None, None, :])
    return np.maximum(t_in, 0.0), t_out


@pytest.mark.parametrize("R", [4, 8, 12, 16])
def test_flat_walk_equals_float64_brute_force(oracle, R, capsys):
    n = 600
    o, d = _family(R, n, seed=5)
    dense = np.random.default_rng(R).random((R, R, R)) < 0.5
    words = TC.pack_words(dense)
    S = 3 * R
    got = oracle.trace(rays_o=o, rays_d=d, R=R, occ=words, mode=1, S=S)
    nh = got["num_hits"]
    assert nh.max() <= S and nh.max() > R // 2 and (nh == 0).any()
    t_in, t_out = _brute_force(o, d, R, dense)
    chord = t_out - t_in
    thr = CHORD_MULTIPLE * EPS * t_out
    crossed = (chord > 0) & dense[None]
    kept = crossed & (chord >= thr)
    left_out = crossed & ~kept
    t0 = got["t_start"].reshape(n, S)
    t1 = got["t_end"].reshape(n, S)
    mid = 0.5 * (got["start"].reshape(n, S, 3).astype(np.float64) + got["end"].reshape(n, S, 3).astype(np.float64))
    n_kept = n_left = 0
    for r in range(n):
        k = int(nh[r])
        cells = np.clip(np.floor((mid[r, :k] + 1.0) * (R / 2.0)).astype(int), 0, R - 1)      # the walk's cell, from the midpoint
        cx, cy, cz = cells[:, 0], cells[:, 1], cells[:, 2]
        assert dense[cx, cy, cz].all(), f"ray {r}: a segment in an empty cell"
        keep = kept[r, cx, cy, cz]
        n_left += int((~keep).sum())
        walk = [tuple(c) for c in cells[keep]]
        bx, by, bz = np.nonzero(kept[r])
        order = np.argsort(t_in[r, bx, by, bz], kind="stable")
        want = list(zip(bx[order].tolist(), by[order].tolist(), bz[order].tolist()))
        assert walk == want, f"ray {r} (o={o[r]}, d={d[r]}): walk {walk} != brute force {want}"
        n_kept += len(want)
        wi, wo = t_in[r, cx, cy, cz][keep], t_out[r, cx, cy, cz][keep]
        assert np.all(np.abs(t0[r, :k][keep] - wi) <= T_MULTIPLE * EPS * wo), f"ray {r}: t_start"
        assert np.all(np.abs(t1[r, :k][keep] - wo) <= T_MULTIPLE * EPS * wo), f"ray {r}: t_end"
    n_left = max(n_left, int(left_out.sum()))
    share = n_left / max(n_kept + n_left, 1)
    with capsys.disabled():
        print(f"\n[flat walk vs float64 brute force, R = {R}] {n} rays, {n_kept} cells compared, {n_left} left out ({100 * share:.3f} %)")
    assert n_kept > 2 * n
    assert share <= 0.01
