"""rtxn_isosurface on the device (include/rtxn.h, "mesh extraction") against the numpy restatement of
tests/_isosurface_reference.py: triangles equal, vertices bit-equal in float32, normals held to the float64 restatement; the
invariants of the DEVICE output computed on the host in float64; capacities, determinism and capture."""
import numpy as np
import pytest

import _isosurface_reference as R

pytestmark = pytest.mark.gpu

BOX = ((-0.7, -1.0, -0.31), (0.9, 0.55, 1.0))       # spacings that float32 does not hold
ISO = 0.37


def _lattices():
    """name -> (lattice + ISO so that every surface sits at iso = 0.37, Euler characteristic, analytic volume in lattice units)"""
    shift = lambda v: (v.astype(np.float64) + ISO).astype(np.float32)     # noqa: E731
    return {
        "corner": (R.corner_lattice(), None, None),
        "sphere": (shift(R.sphere_lattice()), 2, 4.0 / 3.0 * np.pi * 27.0),
        "torus": (shift(R.torus_lattice()), 0, 2.0 * np.pi ** 2 * 3.6 * 1.45 ** 2),
        "ellipsoid67": (shift(R.ellipsoid_lattice((3, 5, 67), (0.8, 1.7, 31.5), (1.1, 2.05, 33.2))), 2, None),
        "ellipsoid130": (shift(R.ellipsoid_lattice((4, 3, 130), (1.3, 0.85, 64.0), (1.45, 1.05, 64.3))), 2, None),
        # 1200 rows (x, y): the row offsets span two groups of 1024
        "slab1200": (shift(R.ellipsoid_lattice((40, 30, 5), (17.5, 12.2, 1.6), (19.3, 14.6, 2.05))), 2, None),
        "noise": (R.noise_lattice(iso=ISO), None, None),
    }


NAMES = ["corner", "sphere", "torus", "ellipsoid67", "ellipsoid130", "slab1200", "noise"]


@pytest.fixture(scope="module")
def cases(gpu):
    """per lattice: the restatements (computed once, never changed) and the device's full result"""
    torch = gpu
    from rtx_nerf_amd import api
    out = {}
    for name, (v, chi, volume) in _lattices().items():
        v32, t32 = R.isosurface(v, ISO, *BOX, dtype=np.float32)
        v64, t64, n64 = R.isosurface(v, ISO, *BOX, dtype=np.float64, normals=True)
        assert np.array_equal(t32, t64)
        dev = torch.from_numpy(v).cuda()
        verts, tris, nrm, counts = api.isosurface(dev, ISO, BOX, normals=True)
        torch.cuda.synchronize()
        out[name] = dict(lattice=v, dev=dev, chi=chi, volume=volume, v32=v32, tris=t32, v64=v64, n64=n64,
                         verts=verts.cpu().numpy(), got_tris=tris.cpu().numpy(), nrm=nrm.cpu().numpy(), counts=counts.cpu().numpy())
    return out


@pytest.mark.parametrize("name", NAMES)
def test_mesh_equals_the_restatement(cases, name):
    c = cases[name]
    print(f"{name}: {len(c['v32'])} vertices, {len(c['tris'])} triangles")
    assert len(c["tris"]) > 0
    assert c["counts"].tolist() == [len(c["v32"]), len(c["tris"]), 0]
    assert c["got_tris"].dtype == np.int32 and np.array_equal(c["got_tris"], c["tris"])
    assert c["verts"].dtype == np.float32 and np.array_equal(c["verts"].view(np.int32), c["v32"].view(np.int32))
    assert np.isfinite(c["verts"]).all() and np.isfinite(c["nrm"]).all()


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_against_float64(cases, name):
    """|grad| = 1 on these distance fields; about 16 roundings of 2^-24 on a unit vector: 4e-6 per component"""
    c = cases[name]
    err = np.abs(c["nrm"].astype(np.float64) - c["n64"]).max()
    print(f"{name}: max normal error {err:.3e}")
    assert err <= 4e-6
    assert np.abs(np.linalg.norm(c["nrm"].astype(np.float64), axis=1) - 1.0).max() <= 4e-6


def _lattice_units(verts):
    lo, hi = np.float32(BOX[0]).astype(np.float64), np.float32(BOX[1]).astype(np.float64)
    return lo, hi


@pytest.mark.parametrize("name", ["sphere", "torus", "ellipsoid67", "ellipsoid130", "slab1200", "noise"])
def test_closed_surfaces_of_the_device_output(cases, name):
    c = cases[name]
    verts, tris = c["verts"].astype(np.float64), c["got_tris"]
    assert R.is_closed_and_oriented(tris)
    if c["chi"] is not None:
        assert R.euler_characteristic(verts, tris) == c["chi"]
    n = c["lattice"].shape
    lo, hi = _lattice_units(verts)
    cell = np.prod((hi - lo) / (np.array(n) - 1.0))
    vol = R.signed_volume(verts, tris) / cell                  # in lattice units
    print(f"{name}: signed volume {vol:.2f} lattice units" + (f", analytic {c['volume']:.2f}" if c["volume"] else ""))
    assert vol > 0
    if c["volume"] is not None:
        assert 0.9 * c["volume"] <= vol <= c["volume"]


def test_open_mesh_ends_on_the_box(cases):
    c = cases["corner"]
    verts, tris = c["verts"].astype(np.float64), c["got_tris"]
    edges = R.boundary_edges(tris)
    assert len(edges) == 6 and not R.is_closed_and_oriented(tris)
    lo, hi = _lattice_units(verts)
    on_face = (np.abs(verts - lo) < 1e-6) | (np.abs(verts - hi) < 1e-6)
    for a, b in edges:
        assert (on_face[a] & on_face[b]).any()


@pytest.mark.parametrize("name", ["torus", "ellipsoid130", "slab1200"])
def test_capacity(gpu, cases, name):
    torch = gpu
    from rtx_nerf_amd import api
    c = cases[name]
    V, T = len(c["v32"]), len(c["tris"])
    for cv, ct in ((V // 3, T // 2), (V, T - 1), (V - 1, T), (0, T), (V + 5, T + 5)):
        guard = 7
        verts = torch.full((cv + guard, 3), -77.0, device="cuda")
        nrm = torch.full((cv + guard, 3), -77.0, device="cuda")
        tris = torch.full((ct + guard, 3), -77, dtype=torch.int32, device="cuda")
        counts = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        api.isosurface(c["dev"], ISO, BOX, normals=True, max_vertices=cv, max_triangles=ct, counts=counts, vertices=verts,
                       triangles=tris, normals_out=nrm)
        torch.cuda.synchronize()
        assert counts.tolist() == [V, T, int(cv < V or ct < T)], (cv, ct)
        kv, kt = min(cv, V), min(ct, T)
        assert np.array_equal(verts[:kv].cpu().numpy().view(np.int32), c["verts"][:kv].view(np.int32))
        assert np.array_equal(nrm[:kv].cpu().numpy().view(np.int32), c["nrm"][:kv].view(np.int32))
        assert np.array_equal(tris[:kt].cpu().numpy(), c["tris"][:kt])          # true vertex ids, past the vertex capacity too
        assert bool((verts[kv:] == -77.0).all()) and bool((nrm[kv:] == -77.0).all()) and bool((tris[kt:] == -77).all()), (cv, ct)
    # counts only: no arrays at all
    counts = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    from rtx_nerf_amd import _lib
    import ctypes as C
    ws = api.isosurface_workspace(c["lattice"].shape)
    a = _lib.IsosurfaceArgs()
    a.density, a.n = c["dev"].data_ptr(), (C.c_int * 3)(*c["lattice"].shape)
    a.lo, a.hi, a.iso = (C.c_float * 3)(*BOX[0]), (C.c_float * 3)(*BOX[1]), ISO
    a.counts, a.workspace, a.workspace_bytes = counts.data_ptr(), ws.data_ptr(), ws.numel() * 4
    _lib.check(_lib.lib().rtxn_isosurface(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rtxn_isosurface")
    torch.cuda.synchronize()
    assert counts.tolist() == [V, T, 1]
    # without normals nothing but vertices and triangles is produced
    verts, tris, none, counts = api.isosurface(c["dev"], ISO, BOX, normals=False)
    assert none is None and np.array_equal(verts.cpu().numpy().view(np.int32), c["verts"].view(np.int32))
    assert np.array_equal(tris.cpu().numpy(), c["tris"])


def test_two_runs_give_the_same_bytes(gpu, cases):
    torch = gpu
    from rtx_nerf_amd import api
    c = cases["noise"]
    again = api.isosurface(c["dev"], ISO, BOX, normals=True)
    torch.cuda.synchronize()
    for got, key in zip(again, ("verts", "got_tris", "nrm", "counts")):
        assert np.array_equal(got.cpu().numpy().view(np.uint8), c[key].view(np.uint8)), key


def test_isosurface_is_capturable(gpu, cases):
    """Captured with fixed capacities; replayed after the lattice was overwritten IN PLACE it equals eager on the new contents."""
    torch = gpu
    from rtx_nerf_amd import api
    first, second = cases["torus"], None
    lattice = first["dev"].clone()
    V, T = 2 * len(first["v32"]), 2 * len(first["tris"])
    buf = dict(counts=torch.zeros(3, dtype=torch.int32, device="cuda"), vertices=torch.zeros((V, 3), device="cuda"),
               triangles=torch.zeros((T, 3), dtype=torch.int32, device="cuda"), normals_out=torch.zeros((V, 3), device="cuda"),
               workspace=api.isosurface_workspace(lattice.shape))
    api.isosurface(lattice, ISO, BOX, max_vertices=V, max_triangles=T, **buf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        api.isosurface(lattice, ISO, BOX, max_vertices=V, max_triangles=T, **buf)
    # the new contents: the torus moved by a node along x and thinned
    new = (R.torus_lattice(centre=(5.1, 5.6, 3.05), r=1.3).astype(np.float64) + ISO).astype(np.float32)
    lattice.copy_(torch.from_numpy(new).cuda())
    for t in buf.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    second = api.isosurface(torch.from_numpy(new).cuda(), ISO, BOX, normals=True)
    nv, nt, over = buf["counts"].tolist()
    assert (nv, nt, over) == (second[0].shape[0], second[1].shape[0], 0) and nv != len(first["v32"])
    assert torch.equal(buf["vertices"][:nv], second[0]) and torch.equal(buf["triangles"][:nt], second[1])
    assert torch.equal(buf["normals_out"][:nv], second[2])
    v_ref, t_ref = R.isosurface(new, ISO, *BOX, dtype=np.float32)
    assert np.array_equal(second[0].cpu().numpy().view(np.int32), v_ref.view(np.int32)) and np.array_equal(second[1].cpu().numpy(), t_ref)
