"""rtxn_isosurface as include/rtxn.h states it, in numpy: isosurface(density, iso, lo, hi, dtype) walks nodes, cubes and tets in
plain Python loops with every operation of the vertex arithmetic rounded in `dtype` -- np.float32 is the restatement the
device output is compared with bit for bit, np.float64 the one normals and invariants are held to.  The case table comes from
tools/gen_tet_table.py, which defines it.  Also here: the lattices of the tests, and the host-side invariants of a mesh
(closedness, Euler characteristic, signed volume, boundary edges), all in float64."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_tet_table  # noqa: E402

EDGE_TYPES = gen_tet_table.EDGE_TYPES
FLT_MAX = np.float32(np.finfo(np.float32).max)


def sanitize(density):
    v = np.asarray(density, dtype=np.float32).copy()
    v[np.isnan(v)] = 0.0
    return np.clip(v, -FLT_MAX, FLT_MAX)


def spacing(n, lo, hi, dtype):
    """(h, P): h_c = (hi_c - lo_c) / (n_c - 1) and P_c(i) = lo_c + i * h_c, each operation rounded in dtype"""
    lo, hi = [np.asarray(np.asarray(b, dtype=np.float32), dtype=dtype) for b in (lo, hi)]
    h = [(hi[c] - lo[c]) / dtype(n[c] - 1) for c in range(3)]
    return h, lambda c, i: lo[c] + dtype(i) * h[c]


def _gradient(v, h, node):
    """central differences of the sanitised lattice at a node, one-sided at the boundary, in float64"""
    g = np.zeros(3)
    for c in range(3):
        i, n = node[c], v.shape[c]
        a, b = list(node), list(node)
        a[c], b[c] = max(i - 1, 0), min(i + 1, n - 1)
        g[c] = (float(v[tuple(b)]) - float(v[tuple(a)])) / ((b[c] - a[c]) * float(h[c]))
    return g


def isosurface(density, iso, lo, hi, dtype=np.float32, normals=False):
    """(vertices dtype[V, 3], triangles int32[T, 3][, normals float64[V, 3]])"""
    v = sanitize(density)
    n = v.shape
    iso = np.float32(iso)
    inside = v > iso
    h, P = spacing(n, lo, hi, dtype)
    _, case = gen_tet_table.tables()
    ids, verts, nrms = {}, [], []
    with np.errstate(all="ignore"):
        for x in range(n[0]):
            for y in range(n[1]):
                for z in range(n[2]):
                    for t, d in enumerate(EDGE_TYPES):
                        q = (x + d[0], y + d[1], z + d[2])
                        if q[0] >= n[0] or q[1] >= n[1] or q[2] >= n[2] or inside[x, y, z] == inside[q]:
                            continue
                        a, b = dtype(v[x, y, z]), dtype(v[q])
                        s = (dtype(iso) - a) / (b - a)
                        s = dtype(0) if not s >= 0 else (dtype(1) if s > 1 else s)
                        ids[(x, y, z, t)] = len(verts)
                        verts.append([P(c, (x, y, z)[c]) + s * (dtype(d[c]) * h[c]) for c in range(3)])
                        if normals:
                            ga, gb = _gradient(v, h, (x, y, z)), _gradient(v, h, q)
                            g = ga + float(s) * (gb - ga)
                            ln = np.sqrt((g * g).sum())
                            nrms.append(-g / ln if ln > 0 else np.zeros(3))
    tris = []
    for x in range(n[0] - 1):
        for y in range(n[1] - 1):
            for z in range(n[2] - 1):
                for k in range(6):
                    mask = 0
                    for i, c in enumerate(gen_tet_table.tet_corners(k)):
                        mask |= int(inside[x + c[0], y + c[1], z + c[2]]) << i
                    for tri in case[k][mask]:
                        tris.append([ids[(x + (c & 1), y + (c >> 1 & 1), z + (c >> 2), t)] for c, t in tri])
    out = (np.array(verts, dtype=dtype).reshape(-1, 3), np.array(tris, dtype=np.int32).reshape(-1, 3))
    return out + (np.array(nrms, dtype=np.float64).reshape(-1, 3),) if normals else out


# ------------------------------------------------------------------------------------------------------------ lattices
def _grid(n):
    return np.meshgrid(*[np.arange(m, dtype=np.float64) for m in n], indexing="ij")


def corner_lattice():
    """(2,2,2), one corner inside: an open mesh"""
    v = np.zeros((2, 2, 2), dtype=np.float32)
    v[1, 1, 1] = 1.0
    return v


def sphere_lattice(n=(9, 9, 9), centre=(4.2, 3.9, 4.1), r=3.0):
    """density = r - |p - centre| in lattice units, inside the sphere where positive; analytic volume 4/3 pi r^3"""
    X = _grid(n)
    return (r - np.sqrt(sum((X[c] - centre[c]) ** 2 for c in range(3)))).astype(np.float32)


def ellipsoid_lattice(n, radii, centre):
    X = _grid(n)
    return (1.0 - np.sqrt(sum(((X[c] - centre[c]) / radii[c]) ** 2 for c in range(3)))).astype(np.float32)


def torus_lattice(n=(13, 12, 7), centre=(6.1, 5.6, 3.05), R=3.6, r=1.45):
    """axis along z; analytic volume 2 pi^2 R r^2"""
    X = _grid(n)
    q = np.sqrt((X[0] - centre[0]) ** 2 + (X[1] - centre[1]) ** 2) - R
    return (r - np.sqrt(q * q + (X[2] - centre[2]) ** 2)).astype(np.float32)


def noise_lattice(n=(6, 7, 8), iso=0.37, seed=5):
    """Gaussian noise with a shell of outside values; some nodes exactly iso, one NaN, one +Inf, one -Inf"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(np.float32)
    v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = (-1.0,) * 6
    for p in ((1, 1, 1), (2, 3, 4), (4, 5, 6), (3, 3, 3), (2, 2, 5)):
        v[p] = np.float32(iso)
    v[2, 4, 3], v[3, 2, 2], v[4, 4, 5] = np.nan, np.inf, -np.inf
    return v


# ---------------------------------------------------------------------------------------------------------- invariants
def directed_edges(triangles):
    t = np.asarray(triangles, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_and_oriented(triangles):
    """every directed edge occurs once and its reverse once"""
    e = directed_edges(triangles)
    fwd = {}
    for a, b in e.tolist():
        fwd[(a, b)] = fwd.get((a, b), 0) + 1
    return all(c == 1 and fwd.get((b, a), 0) == 1 for (a, b), c in fwd.items())


def euler_characteristic(vertices, triangles):
    used = np.unique(np.asarray(triangles))
    e = np.sort(directed_edges(triangles), axis=1)
    return len(used) - len(np.unique(e, axis=0)) + len(triangles)


def signed_volume(vertices, triangles):
    p = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def boundary_edges(triangles):
    """undirected edges with exactly one triangle"""
    e = np.sort(directed_edges(triangles), axis=1)
    u, c = np.unique(e, axis=0, return_counts=True)
    return u[c == 1]
