"""Device-free checks that go with tests/test_gpu_trace_hierarchy.py: the case matrix covers what it must, and the
argument checks that rtxn_trace_grid and the two occupancy builders make BEFORE they look for a device refuse what the
ABI promises to refuse, naming the argument.  (The sub_rays checks come after the device check: they are gpu tests.)"""
import ctypes as C

import numpy as np
import pytest

from tools import _trace_cases as TC


def test_matrix_covers_every_axis_value_and_required_combination():
    m = TC.matrix()
    assert {c.R for c in m} == set(TC.GRID_SIZES) and {c.occ for c in m} == set(TC.OCC_FAMILIES)
    assert {c.rays for c in m} == set(TC.RAY_FAMILIES) and {c.levels for c in m} == set(TC.LEVELS)
    assert {c.sub_rays for c in m} == set(TC.SUB_RAYS)
    has = lambda **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in m)   # noqa: E731
    for Q in (2, 64):
        assert has(R=128, levels=TC.FULL, sub_rays=Q, occ="lego", rays="pinhole_out")
    for R in (256, 272, 320, 400, 416):
        for Q in (0, 8):
            assert has(R=R, levels=TC.FULL, sub_rays=Q)
    for R in (16, 128):
        for lv in TC.LEVELS:
            assert has(R=R, levels=lv, rays="lattice") and has(R=R, levels=lv, rays="zero_comp")
    for R in TC.GRID_SIZES:
        assert R < 8 or R % 4 or has(R=R, occ="checker4")
        assert R < 32 or R % 16 or has(R=R, occ="checker16")
    for R in (128, 416):
        assert any(c.R == R and "super" in c.levels and c.rays in ("pinhole_in", "inside_blocks") for c in m)
    assert TC.staging(256) == (True, True) and TC.staging(272) == (False, True) and TC.staging(400) == (False, True)
    assert TC.staging(416) == (False, False)
    d = np.random.default_rng(0).random((20, 20, 20)) < 0.3
    from rtx_nerf_amd import scenes
    np.testing.assert_array_equal(TC.pack_words(d), scenes.pack_occupancy(d))


def _fake(n=8):
    """A non-NULL pointer that is never dereferenced: every call below is refused on its arguments alone (and asks for
    zero rays, so that nothing could be launched even if it were not)."""
    return C.c_void_p(0x1000 * n)


def _params(**kw):
    from rtx_nerf_amd import _lib
    p = _lib.TraceParams()
    p.look_at, p.width, p.height, p.ray_count, p.mode, p.num_hits = _fake(1), 8, 8, 0, 1, _fake(2)
    p.focal_length = p.aspect_ratio = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw,word", [
    (dict(grid_res=6, occupancy=_fake(3), occupancy_coarse=_fake(4)), b"occupancy_coarse"),                   # R % 4 != 0
    (dict(grid_res=20, occupancy=_fake(3), occupancy_coarse=_fake(4)), None),                                  # control: accepted so far
    (dict(grid_res=16, occupancy_coarse=_fake(4)), b"occupancy_coarse"),                                      # coarse without occupancy
    (dict(grid_res=20, occupancy=_fake(3), occupancy_coarse=_fake(4), occupancy_super=_fake(5)), b"occupancy_super"),   # R % 16 != 0
    (dict(grid_res=24, occupancy=_fake(3), occupancy_coarse=_fake(4), occupancy_super=_fake(5)), b"occupancy_super"),
    (dict(grid_res=16, occupancy=_fake(3), occupancy_super=_fake(5)), b"occupancy_super"),                    # super without coarse
    (dict(grid_res=16, occupancy=_fake(3), occupancy_bricks=_fake(6)), b"occupancy_bricks"),                  # bricks without coarse
    (dict(grid_res=16, occupancy=_fake(3), occupancy_bricks=_fake(6), occupancy_super=_fake(5)), b"occupancy_bricks"),
])
def test_trace_grid_refuses_inconsistent_hierarchy_before_any_device_use(kw, word):
    import torch
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    p = _params(**kw)
    rc = lib.rtxn_trace_grid(C.byref(p), None)
    if word is None:       # passes the argument checks: ends at the device check (2) or, with a device, at ray_count == 0 (0)
        assert rc == (0 if torch.cuda.is_available() else 2)
        return
    assert rc == 1, "RTXN_ERR_INVALID, with or without a device"
    assert word in lib.rtxn_last_error()


@pytest.mark.parametrize("R", [0, 2, 6, 1028, -4])
@pytest.mark.parametrize("entry", ["rtxn_build_occupancy_mip", "rtxn_build_occupancy_bricks"])
def test_occupancy_builders_refuse_bad_grid_res_before_any_device_use(entry, R):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    rc = getattr(lib, entry)(_fake(1), R, _fake(2), None)
    assert rc == 1
    msg = lib.rtxn_last_error()
    assert entry.encode() in msg and b"grid_res" in msg and str(R).encode() in msg
    assert getattr(lib, entry)(None, 16, _fake(2), None) == 1 and b"NULL" in lib.rtxn_last_error()
