"""The restatement the device isosurface is held to (tests/_isosurface_reference.py), checked on its own without a GPU: the
committed case table is the generator's output, the restatement's meshes have the invariants the rule promises on the lattices
the GPU tests use, a linear field puts every vertex on its plane, and write_ply round-trips."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import _isosurface_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE_UNITS = lambda n: ((0.0, 0.0, 0.0), tuple(float(m - 1) for m in n))      # noqa: E731


def test_committed_table_is_the_generators_output():
    import gen_tet_table
    assert open(os.path.join(ROOT, "rtx_nerf_amd", "csrc", "tet_table.h")).read() == gen_tet_table.header_text()
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tet_table.py"), "--check"]).returncode == 0
    assert '#include "tet_table.h"' in open(os.path.join(ROOT, "rtx_nerf_amd", "csrc", "mesh.hip")).read()


def test_the_split_and_the_cases():
    import gen_tet_table as G
    corner, case = G.tables()
    assert corner == [[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]]
    # the six tets fill the cube: their volumes are 1/6 each, with alternating handedness
    for k in range(6):
        c = np.array(G.tet_corners(k), dtype=np.float64)
        assert abs(np.linalg.det(c[1:] - c[0])) == pytest.approx(1.0)
    for k in range(6):
        for mask in range(16):
            inside = bin(mask).count("1")
            assert len(case[k][mask]) == (0, 1, 2, 1, 0)[inside]
            for tri in case[k][mask]:
                assert len(set(tri)) == 3
                for c, t in tri:                          # every vertex lies on an edge of the tet that the mask cuts
                    d = G.EDGE_TYPES[t]
                    other = c + (d[0] | d[1] << 1 | d[2] << 2)
                    assert c in corner[k] and other in corner[k]
                    assert (mask >> corner[k].index(c) & 1) != (mask >> corner[k].index(other) & 1)
            # complementing the mask keeps the triangles and flips their winding
            flipped = [(a, c, b) for a, b, c in case[k][15 - mask]]
            assert sorted(sorted(t) for t in flipped) == sorted(sorted(t) for t in case[k][mask])


CLOSED = {
    "sphere": (lambda: R.sphere_lattice(), 0.0, 2, 4.0 / 3.0 * np.pi * 27.0),
    "torus": (lambda: R.torus_lattice(), 0.0, 0, 2.0 * np.pi ** 2 * 3.6 * 1.45 ** 2),
    "ellipsoid67": (lambda: R.ellipsoid_lattice((3, 5, 67), (0.8, 1.7, 31.5), (1.1, 2.05, 33.2)), 0.0, 2, 4.0 / 3.0 * np.pi * 0.8 * 1.7 * 31.5),
    "ellipsoid130": (lambda: R.ellipsoid_lattice((4, 3, 130), (1.3, 0.85, 64.0), (1.45, 1.05, 64.3)), 0.0, 2, 4.0 / 3.0 * np.pi * 1.3 * 0.85 * 64.0),
    "slab1200": (lambda: R.ellipsoid_lattice((40, 30, 5), (17.5, 12.2, 1.6), (19.3, 14.6, 2.05)), 0.0, 2, None),
    "noise": (lambda: R.noise_lattice(), 0.37, None, None),
}


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_lattices(name):
    make, iso, chi, volume = CLOSED[name]
    v = make()
    verts, tris = R.isosurface(v, iso, *LATTICE_UNITS(v.shape), dtype=np.float64)
    assert len(tris) > 0 and np.isfinite(verts).all()
    assert tris.min() == 0 and tris.max() == len(verts) - 1
    assert R.is_closed_and_oriented(tris)
    vol = R.signed_volume(verts, tris)
    assert vol > 0                                       # outward is towards lower density
    if chi is not None:
        assert R.euler_characteristic(verts, tris) == chi
    if name in ("sphere", "torus"):                      # the thin ellipsoids are too coarse for a volume bound
        assert 0.9 * volume <= vol <= volume
    # the float32 restatement has the same connectivity, and its vertices are the float64 ones to rounding
    v32, t32 = R.isosurface(v, iso, *LATTICE_UNITS(v.shape), dtype=np.float32)
    assert v32.dtype == np.float32 and np.array_equal(t32, tris)
    if name != "noise":                                  # (its +-FLT_MAX nodes overflow b - a in float32 only)
        assert np.abs(v32 - verts).max() <= 130 * 4 * 2.0 ** -24


def test_open_mesh_ends_on_the_box():
    v = R.corner_lattice()
    lo, hi = (-0.7, -1.0, -0.31), (0.9, 0.55, 1.0)
    verts, tris = R.isosurface(v, 0.37, lo, hi, dtype=np.float64)
    assert len(verts) == 7 and len(tris) == 6            # the 7 edge types into corner (1,1,1); one triangle per tet
    edges = R.boundary_edges(tris)
    assert len(edges) == 6
    on_face = (np.abs(verts - np.float32(lo)) < 1e-6) | (np.abs(verts - np.float32(hi)) < 1e-6)
    for a, b in edges:
        assert (on_face[a] & on_face[b]).any()


def test_linear_field_vertices_lie_on_the_plane():
    n, lo, hi = (7, 6, 9), (-0.7, -1.0, -0.31), (0.9, 0.55, 1.0)
    w, iso = np.array([0.83, -1.27, 0.55]), 0.137
    h, P = R.spacing(n, lo, hi, np.float64)
    X = np.meshgrid(*[np.array([P(c, i) for i in range(n[c])]) for c in range(3)], indexing="ij")
    field = (w[0] * X[0] + w[1] * X[1] + w[2] * X[2]).astype(np.float32)
    verts, tris = R.isosurface(field, iso, lo, hi, dtype=np.float32)
    assert len(tris) > 20
    # the lattice holds the field rounded to float32: 2^-24 relative on values of size <= sum |w_c| max |p_c|; t adds three
    # roundings and the position two more on coordinates of size <= 1: the plane's residual, in units of the field, stays
    # within 4 x 2^-24 relative to the field's size sum |w_c| (|p_c| <= 1).
    scale = float(np.abs(w).sum())
    assert np.abs(verts.astype(np.float64) @ w - iso).max() <= 4 * 2.0 ** -24 * scale


def _read_ply(path):
    """binary little-endian PLY with float vertex properties and one uchar/int face list"""
    with open(path, "rb") as f:
        assert f.readline() == b"ply\n" and f.readline() == b"format binary_little_endian 1.0\n"
        counts, props = {}, {}
        while True:
            w = f.readline().split()
            if w[0] == b"end_header":
                break
            if w[0] == b"element":
                cur = w[1].decode()
                counts[cur], props[cur] = int(w[2]), []
            elif w[0] == b"property":
                props[cur].append(b" ".join(w[1:]).decode())
        assert all(p.startswith("float ") for p in props["vertex"]) and props["face"] == ["list uchar int vertex_indices"]
        k = len(props["vertex"])
        vert = np.frombuffer(f.read(4 * k * counts["vertex"]), dtype="<f4").reshape(-1, k)
        faces = []
        for _ in range(counts["face"]):
            assert struct.unpack("<B", f.read(1))[0] == 3
            faces.append(struct.unpack("<3i", f.read(12)))
        assert f.read() == b""
    return [p.split()[1] for p in props["vertex"]], vert, np.array(faces, dtype=np.int32).reshape(-1, 3)


def test_write_ply_round_trips(tmp_path):
    from rtx_nerf_amd import api
    v = R.sphere_lattice()
    verts, tris, nrm = R.isosurface(v, 0.0, (-0.7, -1.0, -0.31), (0.9, 0.55, 1.0), dtype=np.float32, normals=True)
    p = str(tmp_path / "m.ply")
    api.write_ply(p, verts, tris, nrm)
    names, vert, faces = _read_ply(p)
    assert names == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(vert[:, :3], verts) and np.array_equal(vert[:, 3:], nrm.astype(np.float32)) and np.array_equal(faces, tris)
    api.write_ply(p, verts, tris)
    names, vert, faces = _read_ply(p)
    assert names == ["x", "y", "z"] and np.array_equal(vert, verts) and np.array_equal(faces, tris)
    api.write_ply(p, verts[:0], tris[:0])
    assert _read_ply(p)[1].shape == (0, 3)
    with pytest.raises(ValueError):
        api.write_ply(p, verts[:5], tris)
