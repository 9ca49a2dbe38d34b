"""Seeded case generators for the traversal: occupancy families, ray families and the matrix that
tests/test_gpu_trace_hierarchy.py walks and tools/fuzz_trace.py draws from.  numpy only (no torch, no GPU), so the
generators and the oracle side of every case can be exercised on a machine without a device.

Staging paths of trace_kernel (rtx_nerf_amd/csrc/trace.hip), from its two constants:
  coarse mip in LDS  iff ceil((R/4)^3 / 32)  <= kCoarseLdsWords = 8192  <=>  R <= 256
  super  mip in LDS  iff ceil((R/16)^3 / 32) <= kSuperLdsWords  = 512   <=>  R <= 400   (R = 400: 489 words)
so R <= 256 stages both, R = 272..400 reads the coarse mip from global memory beside a staged super mip, and
R >= 416 reads both from global memory.
"""
import collections
import functools
import itertools

import numpy as np

from rtx_nerf_amd import scenes

K_COARSE_LDS_WORDS = 8192
K_SUPER_LDS_WORDS = 512

LEVELS = {            # name -> (coarse, super, bricks)
    "flat": (False, False, False),
    "coarse": (True, False, False),
    "coarse+bricks": (True, False, True),
    "coarse+super": (True, True, False),
    "coarse+super+bricks": (True, True, True),
}
SUB_RAYS = (0, 2, 8, 64)
GRID_SIZES = (4, 16, 20, 48, 128, 256, 272, 320, 400, 416, 1024)
OCC_FAMILIES = ("zeros", "ones", "corners", "mid_super", "checker4", "checker16", "shell", "bern01", "bern1", "bern30", "lego")
RAY_FAMILIES = ("pinhole_out", "pinhole_in", "inside_blocks", "window", "random", "zero_comp", "lattice", "grazing", "backwards")

Case = collections.namedtuple("Case", "R occ rays levels sub_rays")


def case_id(c):
    return f"R{c.R}-{c.occ}-{c.rays}-{c.levels}-Q{c.sub_rays}"


def staging(R):
    """(coarse staged in LDS, super staged in LDS) for a grid of R^3 cells."""
    return ((R // 4) ** 3 + 31) // 32 <= K_COARSE_LDS_WORDS, 0 < ((R // 16) ** 3 + 31) // 32 <= K_SUPER_LDS_WORDS


def levels_allowed(R, levels):
    coarse, sup, _ = LEVELS[levels]
    return (not coarse or R % 4 == 0) and (not sup or R % 16 == 0)


def pack_words(dense):
    """bool[R,R,R] -> uint32 words, bit ((x*R+y)*R+z), LSB first: scenes.pack_occupancy without its 4-byte-per-cell
    temporaries (416^3 cells)."""
    b = np.packbits(np.ascontiguousarray(dense, dtype=bool).reshape(-1), bitorder="little")
    pad = (-b.size) % 4
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    return b.view("<u4").astype(np.uint32, copy=False)


# ----------------------------------------------------------------------------- occupancy
def _checker_words_1024(block):
    """3-D checkerboard of block^3 cells at R = 1024, written as words (a z-row is 32 words; no 1-GiB bool array)."""
    R = 1024
    run = {4: (0x0F0F0F0F, 0xF0F0F0F0), 16: (0x0000FFFF, 0xFFFF0000)}[block]
    par = ((np.arange(R) // block)[:, None] + (np.arange(R) // block)[None, :]) & 1
    rows = np.where(par == 0, np.uint32(run[0]), np.uint32(run[1])).astype(np.uint32)
    return np.ascontiguousarray(np.broadcast_to(rows[:, :, None], (R, R, R // 32))).reshape(-1)


@functools.lru_cache(maxsize=3)
def occupancy(family, R, seed=0):
    """-> (dense bool[R,R,R] or None at R = 1024, words uint32[ceil(R^3/32)])."""
    rng = np.random.default_rng([seed, R, OCC_FAMILIES.index(family)])
    n = R ** 3
    if R == 1024:
        if family in ("checker4", "checker16"):
            return None, _checker_words_1024(int(family[7:]))
        words = np.zeros(n // 32, np.uint32)
        if family == "zeros":
            return None, words
        if family not in ("bern01", "corners"):
            raise ValueError(f"{family}: not built at R = 1024")
        if family == "bern01":
            idx = np.unique(rng.integers(0, n, n // 1000))
        else:
            c = np.array(list(itertools.product((0, R - 1), repeat=3)))
            idx = (c[:, 0] * R + c[:, 1]) * R + c[:, 2]
        np.bitwise_or.at(words, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
        return None, words
    dense = np.zeros((R, R, R), bool)
    ax = np.arange(R)
    if family == "zeros":
        pass
    elif family == "ones":
        dense[:] = True
    elif family == "corners":
        for c in itertools.product((0, R - 1), repeat=3):
            dense[c] = True
    elif family == "mid_super":
        # one cell in the middle of every other 16^3 block (of the single middle cell of a grid smaller than that)
        if R < 32:
            dense[R // 2, R // 2, R // 2] = True
        else:
            nb = R // 16
            for X, Y, Z in itertools.product(range(nb), repeat=3):
                if (X + Y + Z) % 2 == 0:
                    dense[16 * X + 8, 16 * Y + 7, 16 * Z + 8] = True
    elif family in ("checker4", "checker16"):
        b = int(family[7:])
        k = ax // b
        dense = ((k[:, None, None] + k[None, :, None] + k[None, None, :]) & 1) == 0
    elif family == "shell":
        c = (ax.astype(np.float32) + 0.5) * (2.0 / R) - 1.0
        r2 = c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2
        dense = np.abs(np.sqrt(r2) - 0.7) <= 1.0 / R
    elif family in ("bern01", "bern1"):
        k = max(1, int(n * (0.001 if family == "bern01" else 0.01)))
        dense.reshape(-1)[rng.integers(0, n, k)] = True
    elif family == "bern30":
        dense = rng.integers(0, 256, (R, R, R), dtype=np.uint8) < 77
    elif family == "lego":                       # its float meshgrids take seconds above 128^3: used up to there
        dense = scenes.lego_standin_density(R, seed=seed + 1)
    else:
        raise ValueError(family)
    dense = np.ascontiguousarray(dense)
    return dense, pack_words(dense)


# ----------------------------------------------------------------------------- rays
def _unit(d):
    d = np.asarray(d, np.float32)
    return (d / np.sqrt((d * d).sum(axis=1, dtype=np.float32))[:, None]).astype(np.float32)


def _plane(i, R):
    """Lattice plane i exactly as the walk computes it: -1 + i*L in float32."""
    L = np.float32(2.0) / np.float32(R)
    return (np.float32(-1.0) + np.asarray(i, np.float32) * L).astype(np.float32)


def _missing_rays():
    """Rays that never enter the grid: pointing away, passing beside it, and parallel to a slab they are outside of."""
    s2 = np.float32(1 / np.sqrt(2))
    o = np.array([[2, 0, 0], [-2, 0.3, 0.1], [0, 0, 1.5], [3, 3, 3], [0.2, 1.5, 0.3], [1.25, 0, -4], [0, -1.0001, 0], [-3, 0, 2.5]], np.float32)
    d = np.array([[1, 0, 0], [-s2, s2, 0], [0, 0, 1], [s2, 0, s2], [1, 0, 0], [0, 0, 1], [0, 0, -1], [1, 0, 0]], np.float32)
    return o, d


LATTICE_TRIPLES = ((1, 1, 0), (1, 1, 1), (1, -2, 0), (4, 1, 0), (-16, 1, 1), (1, 0, 1), (2, 1, -1), (16, 4, 1), (1, -1, 4), (3, 3, -1))


def rays(family, R, seed=0, dense=None):
    """-> dict for oracle.trace / api.trace_grid: look_at, focal, W, H (pinhole families; ray_begin, ray_count,
    window_chunk, window_stride for "window") or rays_o, rays_d (explicit families).  `cannot_miss`: every ray of the
    family crosses the grid, so a case over a dense occupancy has no ray without hits."""
    rng = np.random.default_rng([seed, R, RAY_FAMILIES.index(family)])
    f = scenes.lego_focal_length(True)
    if family == "pinhole_out":
        return dict(look_at=scenes.pose_spherical(50.0, -35.0, origin_scale=10.0), focal=f, W=48, H=40, cannot_miss=False)
    if family == "pinhole_in":       # translation / 10 at ray generation: the camera sits at radius 0.403, inside the grid
        return dict(look_at=scenes.pose_spherical(-70.0, -25.0, origin_scale=1.0), focal=f, W=48, H=40, cannot_miss=True)
    if family == "backwards":        # negative focal: the rays leave through the back of the camera
        return dict(look_at=scenes.pose_spherical(30.0, -30.0, origin_scale=1.0), focal=scenes.lego_focal_length(False), W=40, H=32,
                    cannot_miss=True)
    if family == "window":           # RowShard(rank 1 of 3).window: rows 1, 4, 7, ... of a 64 x 48 launch
        W, H, world, rank = 64, 48, 3, 1
        return dict(look_at=scenes.pose_spherical(-40.0, -20.0, origin_scale=10.0), focal=f, W=W, H=H, ray_begin=rank * W,
                    ray_count=((H - rank + world - 1) // world) * W, window_chunk=W, window_stride=world * W, cannot_miss=False)
    L = np.float32(2.0) / np.float32(R)
    if family == "random":
        n = 1500 if R <= 416 else 40
        o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
        d = _unit(rng.standard_normal((n, 3)))
        o[: n // 4] = rng.uniform(-1, 1, (n // 4, 3)).astype(np.float32)      # origins inside
        aim = slice(n // 4, n // 2)                                          # aimed at the grid: hits from outside
        d[aim] = _unit(rng.uniform(-0.9, 0.9, (n // 2 - n // 4, 3)).astype(np.float32) - o[aim])
    elif family == "inside_blocks":
        # origins inside an empty 16^3 block and inside an occupied cell (where the occupancy has them), random directions
        pts = [rng.uniform(-0.9, 0.9, 3)]
        if dense is not None:
            if R % 16 == 0:
                sup = dense.reshape(R // 16, 16, R // 16, 16, R // 16, 16).any(axis=(1, 3, 5))
                empty = np.argwhere(~sup)
                if len(empty):
                    b = empty[len(empty) // 2]
                    pts.append(-1.0 + (16 * b + 8.37) * (2.0 / R))
                    pts.append(-1.0 + (16 * b + 8) * (2.0 / R))                # on a lattice corner inside the empty block
            on = np.argwhere(dense)
            if len(on):
                pts.append(-1.0 + (on[len(on) // 2] + 0.41) * (2.0 / R))
        n = 400
        o = np.concatenate([np.tile(np.asarray(p, np.float32), (n, 1)) for p in pts])
        d = _unit(rng.standard_normal((o.shape[0], 3)))
    elif family == "zero_comp":
        os_, ds_ = [], []
        for zero_axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
            for rep in range(40):
                d = rng.uniform(0.2, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
                for a in zero_axes:
                    d[a] = 0.0 if rep % 4 else -0.0
                o = rng.uniform(-1, 1, 3)
                if rep % 2:                                                   # the parallel axes on a lattice plane
                    for a in zero_axes:
                        o[a] = _plane(rng.integers(0, R + 1), R)
                if rep % 5 == 0:                                              # from outside, along a moving axis
                    a = [x for x in range(3) if x not in zero_axes][0]
                    o[a] = -2.5 if d[a] > 0 else 2.5
                os_.append(o)
                ds_.append(d)
        o = np.asarray(os_, np.float32)
        d = np.asarray(ds_, np.float64)
        z = d == 0
        d = _unit(d)
        d[z] = np.asarray(ds_, np.float32)[z]                                 # keep the exact +-0
    elif family == "lattice":
        os_, ds_ = [], []
        for t in LATTICE_TRIPLES:
            for perm in set(itertools.permutations(t)):
                for sg in itertools.product((1, -1), repeat=3):
                    dd = np.array(perm, np.float32) * np.array(sg, np.float32)
                    for mult in (1, 4, 16):
                        hi = R // mult
                        i = rng.integers(0, hi + 1, 3) * mult if hi >= 1 else rng.integers(0, R + 1, 3)
                        os_.append(_plane(i, R))
                        ds_.append(dd)
        sel = rng.permutation(len(os_))[:2400 if R <= 416 else 48]
        o = np.asarray(os_, np.float32)[sel]
        d = _unit(np.asarray(ds_, np.float32)[sel])
    elif family == "grazing":
        os_, ds_ = [], []
        for a in range(3):                                                    # lying in a face of the grid
            for face in (-1.0, 1.0):
                for rep in range(30):
                    b, c = [x for x in range(3) if x != a]
                    o = np.zeros(3)
                    d = np.zeros(3)
                    o[a] = face
                    ang = rng.uniform(0, 2 * np.pi)
                    d[b], d[c] = np.cos(ang), np.sin(ang)
                    o[b], o[c] = (rng.uniform(-1, 1, 2) if rep % 2 else np.array([-2.0 * d[b], -2.0 * d[c]]) + rng.uniform(-0.5, 0.5, 2))
                    if rep % 3 == 0:
                        d[b], d[c] = rng.choice([-1.0, 1.0]), 0.0            # along a lattice line of the face
                        o[c] = _plane(rng.integers(0, R + 1), R)
                    os_.append(o)
                    ds_.append(d)
        for rep in range(240):                                                # entering exactly through an edge or a corner
            tgt = rng.choice([-1.0, 1.0], 3)
            dd = -tgt.copy()
            if rep % 2:                                                       # edge: one coordinate free, on or off the lattice
                a = rng.integers(0, 3)
                tgt[a] = _plane(rng.integers(0, R + 1), R) if rep % 4 == 1 else rng.uniform(-1, 1)
                dd[a] = 0.0 if rep % 8 < 4 else rng.uniform(-0.5, 0.5)
            k = float(rng.choice([1.0, 2.0, 0.5]))                            # o = tgt - k*dd: exact in float32 for these k
            os_.append(tgt - k * dd)
            ds_.append(dd)
        o = np.asarray(os_, np.float32)
        d = _unit(np.asarray(ds_, np.float32))
    else:
        raise ValueError(family)
    mo, md = _missing_rays()
    return dict(rays_o=np.ascontiguousarray(np.concatenate([o, mo]), dtype=np.float32),
                rays_d=np.ascontiguousarray(np.concatenate([d, md]), dtype=np.float32), cannot_miss=False)


def n_rays(r):
    if "look_at" in r:
        return r.get("ray_count", r["W"] * r["H"])
    return r["rays_o"].shape[0]


def oracle_kwargs(r):
    """The ray arguments of oracle.trace (aspect 1.0, as api.trace_grid is called by the tests)."""
    return {k: v for k, v in r.items() if k != "cannot_miss"}


# ----------------------------------------------------------------------------- the matrix
ALL_LEVELS = tuple(LEVELS)
FULL = "coarse+super+bricks"


def matrix():
    """The cases of tests/test_gpu_trace_hierarchy.py, ordered by (R, occupancy) so that a grid is built once."""
    cases = []
    q = itertools.cycle(SUB_RAYS)

    def add(R, occ, rays_, levels, sub_rays=None):
        if not levels_allowed(R, levels):
            raise ValueError(f"{levels} at R = {R}")
        c = Case(R, occ, rays_, levels, next(q) if sub_rays is None else sub_rays)
        if c not in cases:
            cases.append(c)

    # R = 4: one coarse cell.  R = 16: one super cell.  R = 20: 125 coarse cells (a tail word), no super level.
    for occ, rf in (("ones", "lattice"), ("corners", "random"), ("zeros", "grazing"), ("bern30", "zero_comp")):
        for lv in ("flat", "coarse", "coarse+bricks"):
            add(4, occ, rf, lv)
    for lv in ("coarse", "coarse+bricks"):
        for occ, rf in (("checker4", "lattice"), ("lego", "pinhole_out"), ("bern30", "zero_comp"), ("corners", "grazing"), ("shell", "random")):
            add(20, occ, rf, lv)
    # lattice and zero-component rays with every level combination at R = 16 and 128
    for R in (16, 128):
        for lv in ALL_LEVELS:
            add(R, "checker4", "lattice", lv)
            add(R, "lego", "zero_comp", lv)
            add(R, "bern1", "lattice", lv)
            add(R, "mid_super", "zero_comp", lv)
    for occ, rf in (("ones", "random"), ("zeros", "lattice"), ("corners", "grazing"), ("shell", "pinhole_in"), ("bern30", "grazing"),
                    ("bern01", "random"), ("bern30", "backwards")):
        add(16, occ, rf, FULL)
        add(16, occ, rf, "coarse+super")
    # R = 48: three super cells per axis, every occupancy family and every ray family
    for occ, rf in (("zeros", "window"), ("ones", "random"), ("corners", "grazing"), ("mid_super", "lattice"), ("checker4", "zero_comp"),
                    ("checker16", "backwards"), ("shell", "pinhole_out"), ("bern01", "pinhole_in"), ("bern1", "inside_blocks"),
                    ("bern30", "window"), ("lego", "random")):
        add(48, occ, rf, FULL)
    for rf, occ in zip(RAY_FAMILIES, ("checker16", "checker4", "mid_super", "lego", "bern1", "shell", "checker16", "checker4", "bern30")):
        add(48, occ, rf, "coarse+super")
        add(48, occ, rf, FULL)
    # R = 128, the bench size: super + bricks with 2 and 64 lanes per ray; camera inside with the super level
    for Q in (2, 64):
        add(128, "lego", "pinhole_out", FULL, Q)
        add(128, "bern1", "window", FULL, Q)
        add(128, "checker16", "random", FULL, Q)
    for Q in SUB_RAYS:
        add(128, "bern1", "pinhole_in", FULL, Q)
        add(128, "mid_super", "inside_blocks", FULL, Q)
    for occ, rf in (("checker4", "grazing"), ("checker16", "lattice"), ("checker16", "inside_blocks"), ("shell", "backwards"),
                    ("bern01", "random"), ("bern30", "window"), ("corners", "grazing"), ("zeros", "random"), ("ones", "pinhole_in")):
        add(128, occ, rf, FULL)
        add(128, occ, rf, "coarse+super")
    # every staging path with the full hierarchy at sub_rays 0 and 8; both checkerboards at every size
    for R in (256, 272, 320, 400, 416):
        for Q in (0, 8):
            add(R, "checker16", "lattice", FULL, Q)
            add(R, "checker4", "random", FULL, Q)
            add(R, "shell", "pinhole_out", FULL, Q)
            add(R, "bern1", "zero_comp", FULL, Q)
        add(R, "mid_super", "grazing", FULL, 2)
        add(R, "shell", "window", FULL, 64)
        add(R, "checker16", "random", "coarse+super", 2)
        add(R, "checker4", "lattice", "coarse+bricks", 64)
        add(R, "bern01", "lattice", "coarse", 8)
    for Q in SUB_RAYS:
        add(416, "bern01", "pinhole_in", FULL, Q)
        add(416, "mid_super", "inside_blocks", FULL, Q)
        add(416, "checker16", "inside_blocks", "coarse+super", Q)
    # the largest grid, with a hierarchy, a few dozen rays
    for occ, rf, lv, Q in (("checker16", "lattice", FULL, 0), ("checker4", "random", FULL, 8), ("bern01", "lattice", FULL, 2),
                           ("bern01", "random", "coarse+super", 64), ("corners", "lattice", "coarse+bricks", 8), ("checker16", "random", "flat", 0)):
        add(1024, occ, rf, lv, Q)
    order = {R: i for i, R in enumerate(GRID_SIZES)}
    return sorted(cases, key=lambda c: (order[c.R], c.occ, c.rays, c.levels, c.sub_rays))


def reference(oracle, case, seed=0):
    """The flat one-thread CPU walk of a case (oracle.trace, mode 1: it never sees a mip, a brick or a piece), in the
    strided layout with S = longest ray + 2 slots, and the checks that keep the case from going vacuous.
    -> (words, rays dict, S, want)."""
    dense, words = occupancy(case.occ, case.R, seed)
    r = rays(case.rays, case.R, seed, dense=dense)
    kw = oracle_kwargs(r)
    cnt = oracle.trace(R=case.R, occ=words, mode=1, count_only=True, **kw)["num_hits"]
    S = max(int(cnt.max()), 1) + 2
    want = oracle.trace(R=case.R, occ=words, mode=1, S=S, **kw)
    nh = want["num_hits"]
    assert np.array_equal(nh, cnt) and nh.shape[0] == n_rays(r)
    assert nh.max() <= S, "the strided comparison would truncate"
    if case.occ == "zeros":
        assert nh.max() == 0
    else:
        assert nh.max() > 0, "no ray of this case hits anything"
    # a family whose origins all lie well inside the grid cannot miss an occupancy that fills space or encloses them
    if not (r["cannot_miss"] and case.occ in ("ones", "bern30", "checker4", "checker16", "shell")):
        assert nh.min() == 0, "no ray of this case is without hits"
    return words, r, S, want


def packed_from_strided(want, S):
    """The packed (CSR) layout of the same walk: every ray's first num_hits slots, in ray order."""
    nh = want["num_hits"].astype(np.int64)
    keep = (np.arange(S)[None, :] < nh[:, None]).reshape(-1)
    idx = np.concatenate([[0], np.cumsum(nh)[:-1]]).astype(np.int32)
    out = {k: want[k].reshape(nh.shape[0] * S, -1)[keep].reshape((-1,) + want[k].shape[1:]) for k in ("start", "end", "t_start", "t_end")}
    out["seg_ray"] = np.repeat(np.arange(nh.shape[0], dtype=np.int32), nh)
    out["indices"] = idx
    out["total"] = int(nh.sum())
    return out
