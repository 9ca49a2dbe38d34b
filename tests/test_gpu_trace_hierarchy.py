"""The traversal's empty-space skip, every level and every staging path, against the oracle's FLAT one-thread walk.

trace_kernel's production configuration is the DDA walk over the 4^3 coarse mip, the 16^3 super mip and the 64-bit
bricks with sub_rays lanes per ray.  Its claim is that this reproduces the flat walk bit for bit; the reference of
every case here is oracle.trace(mode=1) over the fine occupancy words alone, never another GPU configuration.  The
cases (tools/_trace_cases.py) cross level combinations, sub_rays 0/2/8/64, the grid sizes at which the LDS staging of
the two mips switches (coarse: R <= 256, super: R <= 400, from kCoarseLdsWords / kSuperLdsWords), occupancy families
that force a skip before and after every occupied block, and ray families with exact plane ties.

The builders (mip, bricks, density -> occupancy) are compared with numpy reductions written here, and the argument
checks that rtxn_trace_grid makes after it has found a device are exercised with legal buffers.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _assert_trace_equal, _dev, _occ_dev, _trace_gpu
from tools import _trace_cases as TC

pytestmark = pytest.mark.gpu

_HIER = {}


def _hierarchy(torch, api, family, R, words):
    """Device copies of one occupancy and of every level built from it (kept for the run of cases that share it)."""
    key = (family, R)
    if key not in _HIER:
        _HIER.clear()
        h = dict(occ=_occ_dev(torch, words), coarse=None, bricks=None, super=None)
        if R % 4 == 0:
            h["coarse"] = api.build_occupancy_mip(h["occ"], R)
            h["bricks"] = api.build_occupancy_bricks(h["occ"], R)
        if R % 16 == 0:
            h["super"] = api.build_occupancy_mip(h["coarse"], R // 4)
        _HIER[key] = h
    return _HIER[key]


def _ray_args(torch, r):
    """(positional arguments of api.trace_grid, ray keywords of api.trace_grid, ray keywords of _trace_gpu)."""
    win = {k: r[k] for k in ("ray_begin", "ray_count", "window_chunk", "window_stride") if k in r}
    if "look_at" in r:
        pos = (_dev(torch, r["look_at"].reshape(16)), r["focal"], 1.0, r["W"], r["H"])
        return pos, win, dict(look_at=r["look_at"], f=r["focal"], W=r["W"], H=r["H"], **win)
    o, d = _dev(torch, r["rays_o"]), _dev(torch, r["rays_d"])
    return (), dict(rays_o=o, rays_d=d), dict(rays_o=r["rays_o"], rays_d=r["rays_d"])


@pytest.mark.parametrize("case", TC.matrix(), ids=TC.case_id)
def test_hierarchical_walk_equals_flat_oracle_walk(gpu, oracle, case):
    torch = gpu
    from rtx_nerf_amd import api
    R, Q = case.R, case.sub_rays
    words, r, S, want = TC.reference(oracle, case)
    assert want["num_hits"].max() <= S
    n = TC.n_rays(r)
    h = _hierarchy(torch, api, case.occ, R, words)
    use_coarse, use_super, use_bricks = TC.LEVELS[case.levels]
    lv = dict(occupancy=h["occ"], occupancy_coarse=h["coarse"] if use_coarse else None,
              occupancy_super=h["super"] if use_super else None, occupancy_bricks=h["bricks"] if use_bricks else None)
    assert (lv["occupancy_coarse"] is not None) == use_coarse and (lv["occupancy_super"] is not None) == use_super
    pos, ray_kw, gpu_kw = _ray_args(torch, r)

    # counting pass: num_hits, and with Q lanes per ray the per-piece counts that the write pass will rely on
    nh = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    sub = torch.full((n * Q,), -7, dtype=torch.int32, device="cuda") if Q > 1 else None
    common = dict(grid_res=R, mode=1, sub_rays=Q, sub_hits=sub, **lv, **ray_kw)
    api.trace_grid(*pos, num_hits=nh, **common)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(nh.cpu().numpy(), want["num_hits"])
    if Q > 1:
        np.testing.assert_array_equal(sub.cpu().numpy().reshape(n, Q).sum(axis=1), want["num_hits"])

    # strided write pass: bit-exact, and every slot past num_hits keeps its fill value
    got = _trace_gpu(torch, api, R=R, mode=1, occ=lv["occupancy"], coarse=lv["occupancy_coarse"], bricks=lv["occupancy_bricks"],
                     occupancy_super=lv["occupancy_super"], S=S, sub_rays=Q, sub_hits=sub, **gpu_kw)
    _assert_trace_equal(got, want)
    unused = np.arange(S)[None, :] >= want["num_hits"][:, None]
    for k in ("start", "end", "t_start", "t_end"):
        assert np.all(got[k].reshape(n, S, -1)[unused] == -2.0), f"{k}: a slot past num_hits was written"

    # packed write pass (count -> scan -> write), a capacity three slots short
    pk = TC.packed_from_strided(want, S)
    idx, total = api.scan_hits(nh)
    P = int(total.item())
    assert P == pk["total"]
    np.testing.assert_array_equal(idx.cpu().numpy(), pk["indices"])
    cap = P - 3 if P > 3 else P
    sp = torch.full((max(P, 1), 3), -2.0, device="cuda")
    ep = torch.full((max(P, 1), 3), -2.0, device="cuda")
    t0 = torch.full((max(P, 1),), -2.0, device="cuda")
    t1 = torch.full((max(P, 1),), -2.0, device="cuda")
    sr = torch.full((max(P, 1),), -1, dtype=torch.int32, device="cuda")
    sv = torch.full((max(P, 1), 2), -9.0, device="cuda")
    sf = torch.full((max(P, 1),), 7, dtype=torch.uint8, device="cuda")
    vd = torch.zeros((n, 2), device="cuda")
    stored = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    nh2 = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    api.trace_grid(*pos, num_hits=nh2, viewing_direction=vd, indices=idx, start_points=sp, end_points=ep, t_start=t0, t_end=t1,
                   seg_ray=sr, seg_view=sv, seg_first=sf, num_stored=stored, segment_capacity=cap if P else 1, **common)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(nh2.cpu().numpy(), want["num_hits"])
    np.testing.assert_array_equal(stored.cpu().numpy(), np.clip(cap - pk["indices"], 0, want["num_hits"]))
    for name, t, ref in (("start", sp, pk["start"]), ("end", ep, pk["end"]), ("t_start", t0, pk["t_start"]),
                         ("t_end", t1, pk["t_end"]), ("seg_ray", sr, pk["seg_ray"])):
        np.testing.assert_array_equal(t.cpu().numpy()[:cap], ref[:cap], err_msg=name)
    first = np.zeros(P, np.uint8)
    first[pk["indices"][want["num_hits"] > 0]] = 1
    np.testing.assert_array_equal(sf.cpu().numpy()[:cap], first[:cap])
    np.testing.assert_array_equal(sv.cpu().numpy()[:cap], vd.cpu().numpy()[pk["seg_ray"][:cap]])
    assert np.all(sp.cpu().numpy()[cap:] == -2.0) and np.all(ep.cpu().numpy()[cap:] == -2.0)
    assert np.all(t0.cpu().numpy()[cap:] == -2.0) and np.all(t1.cpu().numpy()[cap:] == -2.0)
    assert np.all(sr.cpu().numpy()[cap:] == -1) and np.all(sv.cpu().numpy()[cap:] == -9.0) and np.all(sf.cpu().numpy()[cap:] == 7)


# ------------------------------------------------------------------ the builders against plain numpy
BUILDER_SIZES = (4, 8, 16, 20, 36, 128, 256, 416, 1024)


def _unpack(words, nbits):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:nbits].astype(bool)


def _builder_occupancy(R):
    """Cells at ~6 % inside half of the 4^3 blocks of 70 % of the 16^3 blocks: on and off blocks at every level.
    -> (dense or None, words); R = 1024 is written as words (a dense bool array would be 1 GiB)."""
    rng = np.random.default_rng(R)
    if R < 1024:
        def up(a, k):
            return np.repeat(np.repeat(np.repeat(a, k, 0), k, 1), k, 2)[:R, :R, :R]
        fine = rng.integers(0, 256, (R, R, R), dtype=np.uint8) < 16
        mid = up(rng.random(((R + 3) // 4,) * 3) < 0.5, 4)
        top = up(rng.random(((R + 15) // 16,) * 3) < 0.7, 16)
        dense = fine & mid & top
        dense[R - 1, R - 1, R - 1] = True          # the last bit of the last word
        return dense, TC.pack_words(dense)
    xyz = rng.integers(0, R, (1_500_000, 3))
    xyz = xyz[((xyz >> 4).sum(axis=1) % 3) != 0]
    idx = np.unique(np.concatenate([(xyz[:, 0] * R + xyz[:, 1]) * R + xyz[:, 2], [R ** 3 - 1]]))
    words = np.zeros(R ** 3 // 32, np.uint32)
    np.bitwise_or.at(words, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    return None, words


def _any_blocks(a):
    r = a.shape[0] // 4
    return a.reshape(r, 4, r, 4, r, 4).any(axis=(1, 3, 5))


def _bricks_ref(dense):
    rc = dense.shape[0] // 4
    b = dense.reshape(rc, 4, rc, 4, rc, 4).transpose(0, 2, 4, 1, 3, 5).reshape(rc ** 3, 64)       # [block][x&3, y&3, z&3]
    w = np.array([((k >> 4) << 4) | (((k >> 2) & 3) << 2) | (k & 3) for k in range(64)], np.uint64)
    return (b.astype(np.uint64) << w).sum(axis=1, dtype=np.uint64)


def _nibbles(words, R):
    """uint8[R, R, R/4]: the four z-cells 4k..4k+3 of every row, from the words alone (R % 8 == 0)."""
    b = np.ascontiguousarray(words).view(np.uint8).reshape(R, R, R // 8)
    return np.stack([b & 15, b >> 4], axis=-1).reshape(R, R, R // 4)


def _coarse_bricks_from_nibbles(nib):
    rc = nib.shape[0] // 4
    nb = nib.reshape(rc, 4, rc, 4, rc)
    coarse = (nb != 0).any(axis=(1, 3))
    bricks = np.zeros((rc, rc, rc), np.uint64)
    for dx in range(4):
        for dy in range(4):
            bricks |= nb[:, dx, :, dy, :].astype(np.uint64) << np.uint64((dx << 4) | (dy << 2))
    return coarse, bricks.reshape(-1)


@pytest.mark.parametrize("R", BUILDER_SIZES)
def test_mip_and_bricks_equal_numpy_reductions(gpu, R):
    torch = gpu
    from rtx_nerf_amd import api
    dense, words = _builder_occupancy(R)
    if dense is not None:
        want_coarse, want_bricks = _any_blocks(dense), _bricks_ref(dense)
    else:
        # the word-level route of the 1024^3 case, first checked against the dense route where both fit
        d128, w128 = _builder_occupancy(128)
        c128, b128 = _coarse_bricks_from_nibbles(_nibbles(w128, 128))
        np.testing.assert_array_equal(c128, _any_blocks(d128))
        np.testing.assert_array_equal(b128, _bricks_ref(d128))
        want_coarse, want_bricks = _coarse_bricks_from_nibbles(_nibbles(words, R))
    rc = R // 4
    assert want_coarse.any() and (rc == 1 or not want_coarse.all())
    occ = _occ_dev(torch, words)
    coarse = api.build_occupancy_mip(occ, R)
    bricks = api.build_occupancy_bricks(occ, R)
    torch.cuda.synchronize()
    got_c = coarse.cpu().numpy().view(np.uint32)
    got_b = bricks.cpu().numpy().view(np.uint64)
    assert got_c.size == (rc ** 3 + 31) // 32 and got_b.size == rc ** 3
    np.testing.assert_array_equal(got_c, TC.pack_words(want_coarse))
    if rc ** 3 % 32:
        assert got_c[-1] >> np.uint32(rc ** 3 % 32) == 0, "unused high bits of the last coarse word"
    np.testing.assert_array_equal(got_b, want_bricks)
    np.testing.assert_array_equal(_unpack(got_c, rc ** 3), got_b != 0)                   # coarse bit == (brick != 0)
    if R % 16 == 0:
        rs = R // 16
        sup = api.build_occupancy_mip(coarse, rc)                                        # the mip of the mip
        torch.cuda.synchronize()
        got_s = sup.cpu().numpy().view(np.uint32)
        want_s = _any_blocks(want_coarse)
        assert got_s.size == (rs ** 3 + 31) // 32 and want_s.any() and (rs < 3 or not want_s.all())
        np.testing.assert_array_equal(got_s, TC.pack_words(want_s))
        if rs ** 3 % 32:
            assert got_s[-1] >> np.uint32(rs ** 3 % 32) == 0, "unused high bits of the last super word"
        np.testing.assert_array_equal(_unpack(got_s, rs ** 3), _any_blocks(_unpack(got_c, rc ** 3).reshape(rc, rc, rc)).reshape(-1))


@pytest.mark.parametrize("threshold", [0.0, 0.5])
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 7, 9, 32, 33, 100])
def test_occupancy_from_density_equals_numpy(gpu, R, threshold):
    """n < 32, n % 32 != 0, a last wave with one word (n % 64 < 32: R = 3, 7, 9) and with two (R = 5, 33), n % 256 != 0;
    NaN, +-Inf, -0.0, denormals and densities exactly at the threshold.  (n % 64 == 32 cannot occur: n is a cube, and no
    cube is 4 mod 8.)  Reference: density > threshold in numpy (NaN is off)."""
    torch = gpu
    from rtx_nerf_amd import _lib, api
    n = R ** 3
    rng = np.random.default_rng(R)
    dens = rng.normal(threshold, 1.0, n).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, threshold, np.nextafter(np.float32(threshold), np.float32(1)),
                        np.nextafter(np.float32(threshold), np.float32(-1))], np.float32)
    where = rng.integers(0, n, max(n // 3, 1))
    dens[where] = special[rng.integers(0, special.size, where.size)]
    tail = min(n, special.size)
    dens[n - tail:] = special[:tail]                # the last cells: the ballot's tail word
    with np.errstate(invalid="ignore"):
        want = dens > np.float32(threshold)
    assert R < 3 or (want.any() and not want.all())
    d_dev = _dev(torch, dens)
    occ = api.occupancy_from_density(d_dev, threshold, R)
    torch.cuda.synchronize()
    got = occ.cpu().numpy().view(np.uint32)
    nwords = (n + 31) // 32
    assert got.size == nwords
    np.testing.assert_array_equal(got, TC.pack_words(want))
    if n % 32:
        assert got[-1] >> np.uint32(n % 32) == 0, "bits at and above n in the last word"
    # through the C entry into a pre-filled, larger buffer: the words are the same and nothing beyond them is written
    buf = torch.full((nwords + 64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rc = _lib.lib().rtxn_occupancy_from_density(C.c_void_p(d_dev.data_ptr()), threshold, R, C.c_void_p(buf.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    b = buf.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(b[:nwords], got)
    assert np.all(b[nwords:] == 0x5a5a5a5a)


# ------------------------------------------------------------------ refusals that come after the device check
@pytest.mark.parametrize("mode,sub_rays,give_sub_hits,word", [(1, 3, True, b"sub_rays"), (1, 6, True, b"sub_rays"), (1, 128, True, b"sub_rays"),
                                                              (1, -1, True, b"sub_rays"), (0, 2, True, b"sub_rays"),
                                                              (1, 8, False, b"sub_hits")])
def test_trace_grid_refuses_bad_sub_rays_and_launches_nothing(gpu, mode, sub_rays, give_sub_hits, word):
    torch = gpu
    from rtx_nerf_amd import _lib, api
    n = 64
    o = torch.zeros((n, 3), device="cuda")
    d = torch.zeros((n, 3), device="cuda")
    o[:, 0] = -2.0
    d[:, 0] = 1.0
    nh = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    sub = torch.full((n * 128,), -7, dtype=torch.int32, device="cuda")
    p = api.trace_params(grid_res=8, rays_o=o, rays_d=d, mode=mode, num_hits=nh, sub_rays=sub_rays,
                         sub_hits=sub if give_sub_hits else None)
    lib = _lib.lib()
    rc = lib.rtxn_trace_grid(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 1 and word in lib.rtxn_last_error()
    torch.cuda.synchronize()
    assert torch.all(nh == -7).item() and torch.all(sub == -7).item()
    with pytest.raises(_lib.RtxnError):
        api.trace_grid(grid_res=8, rays_o=o, rays_d=d, mode=mode, num_hits=nh, sub_rays=sub_rays, sub_hits=sub if give_sub_hits else None)
    # the same launch with a legal lane count runs
    sub_ok = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    api.trace_grid(grid_res=8, rays_o=o, rays_d=d, mode=1, num_hits=nh, sub_rays=8, sub_hits=sub_ok)
    torch.cuda.synchronize()
    assert torch.all(nh == 8).item()
