"""rtxn_density_lattice and Trainer.extract_mesh on the device (include/rtxn.h, "mesh extraction").

The lattice is compared bit for bit with sigma obtained by calling the segment entries the lattice itself uses on numpy-built
pseudo-segments -- the float32 arithmetic the header states -- on the models of test_gpu_occupancy_refresh.py."""
import numpy as np
import pytest

from test_gpu_occupancy_refresh import HGD, Model, _sphere_occ

pytestmark = pytest.mark.gpu

F = np.float32
BOX = ((-0.7, -1.0, -0.31), (0.9, 0.55, 1.0))
SCALE = 37.0


def ref_segments(n, lo, hi):
    """start, end float32[runs][3]: h = (hi - lo) / (n - 1); P(i) = lo + i * h; end_z = start_z + 32 h_z; run g = (x n_y + y) NK + k"""
    lo, hi = np.asarray(lo, dtype=F), np.asarray(hi, dtype=F)
    h = [(hi[c] - lo[c]) / F(n[c] - 1) for c in range(3)]
    nk = (n[2] + 31) // 32
    g = np.arange(n[0] * n[1] * nk, dtype=np.int64)
    k, row = g % nk, g // nk
    x, y = row // n[1], row % n[1]
    start = np.stack([lo[c] + i.astype(F) * h[c] for c, i in enumerate((x, y, 32 * k))], axis=1).astype(F)
    end = start.copy()
    end[:, 2] = start[:, 2] + F(32.0) * h[2]
    return start, end, nk


def ref_lattice(m, n, lo, hi, scale):
    start, end, nk = ref_segments(n, lo, hi)
    s = m.sigma(start, end).astype(F)                       # [runs][32]
    s = np.where(np.isnan(s), F(0), s) * F(scale)
    return s.reshape(n[0], n[1], nk * 32)[:, :, :n[2]]


@pytest.fixture(scope="module")
def models(gpu):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = Model(gpu, kind)
        return cache[kind]
    return get


@pytest.mark.parametrize("kind", ["hash", "freq"])
@pytest.mark.parametrize("n", [(5, 4, 33), (3, 3, 70), (4, 4, 32)])
def test_lattice_is_bit_exact_for_every_pass_size(gpu, models, kind, n):
    """(5,4,33): a tail run of one node; (3,3,70): three runs per row, the last of 6 nodes; (4,4,32): exactly one run per row"""
    torch = gpu
    m = models(kind)
    api = m.api
    want = ref_lattice(m, n, *BOX, SCALE)
    assert np.isfinite(want).all() and len(np.unique(want)) > 16
    runs = api.density_lattice_runs(n)
    for P in (runs, 7):
        out = torch.full(n, -5.0, device="cuda")
        got = api.density_lattice(m.net, grid=m.hg, table=m.table, resolution=n, aabb=BOX, scale=SCALE, out=out, runs_per_pass=P)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == n
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (kind, n, P)
    # the whole cube, a scalar resolution, buffers made by the call
    cube = api.density_lattice(m.net, grid=m.hg, table=m.table, resolution=9, scale=2.0)
    assert np.array_equal(cube.cpu().numpy().view(np.int32), ref_lattice(m, (9, 9, 9), (-1, -1, -1), (1, 1, 1), 2.0).view(np.int32))


def test_unsupported_models(gpu):
    from rtx_nerf_amd import _lib, api
    # a pre-encoded model without a grid, and a grid with 4 features per level: no fused inference kernel
    ext = api.Network(n_neurons=64, n_hidden_layers=4, n_encoded_features=32)
    with pytest.raises(_lib.RtxnError, match=r"status 3.*no fused inference kernel"):
        api.density_lattice(ext, resolution=8)
    odd = api.HashGrid(2, 4, 12, 4, 1.5, n_dir_freqs=4)
    table = gpu.zeros(odd.n_params(), dtype=gpu.float16, device="cuda")
    with pytest.raises(_lib.RtxnError, match=r"status 3.*no fused inference kernel"):
        api.density_lattice(ext, grid=odd, table=table, resolution=8)


def _trainer(torch, encoding, **kw):
    from rtx_nerf_amd.train import Trainer
    R, B = 32, 24 * 24
    model = dict(n_neurons=64, n_hidden_layers=4, hashgrid=HGD) if encoding == "hash" else dict(n_neurons=64, n_hidden_layers=2, n_dir_freqs=12)
    return Trainer(R, _sphere_occ(torch, R), encoding=encoding, batch_rays=B, max_segments=B * 40, lr=1e-2, density_scale=100.0, seed=1,
                   **model, **kw)


def _steps(torch, tr, n=3):
    from rtx_nerf_amd import scenes
    from rtx_nerf_amd.train import camera_rays
    o, d = camera_rays(scenes.pose_spherical(25.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), 24, 24)
    tgt = torch.full((24 * 24, 3), 0.4, device="cuda")
    for _ in range(n):
        tr.step(o, d, tgt)


def _read_ply(path, with_normals):
    with open(path, "rb") as f:
        head = f.read().split(b"end_header\n", 1)
    nv = int(head[0].split(b"element vertex ")[1].split()[0])
    nf = int(head[0].split(b"element face ")[1].split()[0])
    k = 6 if with_normals else 3
    vert = np.frombuffer(head[1][:4 * k * nv], dtype="<f4").reshape(nv, k)
    faces = np.frombuffer(head[1][4 * k * nv:], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    assert len(faces) == nf and (faces["n"] == 3).all()
    return vert, faces["v"]


@pytest.mark.parametrize("encoding", ["hash", "freq"])
def test_extract_mesh_is_isosurface_of_density_lattice(gpu, tmp_path, encoding):
    torch = gpu
    from rtx_nerf_amd import api
    tr = _trainer(torch, encoding)
    _steps(torch, tr)
    n, box = (20, 18, 35), ((-0.8, -0.9, -1.0), (0.85, 0.7, 0.95))
    if encoding != "hash":
        tr.sync_inference_weights()
    lattice = api.density_lattice(tr.net, grid=tr.hg, table=tr.table if encoding == "hash" else None, resolution=n, aabb=box,
                                  scale=tr.density_scale)
    iso = float(lattice.median().item())
    want = api.isosurface(lattice, iso, box, normals=True)
    v, t, nrm = tr.extract_mesh(n, iso=iso, aabb=box)
    assert t.shape[0] > 100 and want[3].tolist() == [v.shape[0], t.shape[0], 0]
    assert torch.equal(v, want[0]) and torch.equal(t, want[1]) and torch.equal(nrm, want[2])
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(nrm).all())
    assert float(v.min()) >= -1.0 and float(v.max()) <= 1.0
    v2, t2, none = tr.extract_mesh(n, iso=iso, aabb=box, normals=False)
    assert none is None and torch.equal(v2, v) and torch.equal(t2, t)
    with pytest.raises(TypeError):
        tr.extract_mesh(n)                                   # iso has no default
    # the PLY written from it reads back equal
    path = str(tmp_path / "mesh.ply")
    api.write_ply(path, v, t, nrm)
    vert, faces = _read_ply(path, True)
    assert np.array_equal(vert[:, :3], v.cpu().numpy()) and np.array_equal(vert[:, 3:], nrm.cpu().numpy())
    assert np.array_equal(faces, t.cpu().numpy())


@pytest.mark.parametrize("encoding", ["hash", "freq"])
def test_extract_mesh_from_the_averaged_weights(gpu, encoding):
    """weights="ema" is the lattice of a fresh model set to ema_parameters()"""
    torch = gpu
    from rtx_nerf_amd import api
    tr = _trainer(torch, encoding, ema_decay=0.9)
    _steps(torch, tr, 5)
    n, box = (12, 11, 34), ((-0.8, -0.9, -1.0), (0.85, 0.7, 0.95))
    got = tr.density_lattice(n, box, weights="ema")
    live = tr.density_lattice(n, box)
    mlp, table = tr.ema_parameters()
    c = tr.net.cfg
    net = api.Network(n_neurons=c.n_neurons, n_hidden_layers=c.n_hidden_layers, n_pos_freqs=c.n_pos_freqs, n_dir_freqs=c.n_dir_freqs,
                      n_pos_dims=c.n_pos_dims, n_dir_dims=c.n_dir_dims, n_output_dims=c.n_output_dims, output_activation=c.output_activation,
                      n_encoded_features=c.n_encoded_features)
    net.set_params(mlp.half())
    want = api.density_lattice(net, grid=tr.hg, table=table.half() if encoding == "hash" else None, resolution=n, aabb=box,
                               scale=tr.density_scale)
    assert torch.equal(got, want) and not torch.equal(got, live)
    iso = float(want.median().item())
    v, t, nrm = tr.extract_mesh(n, iso=iso, aabb=box, weights="ema")
    ref = api.isosurface(want, iso, box)
    assert t.shape[0] > 0 and torch.equal(v, ref[0]) and torch.equal(t, ref[1]) and torch.equal(nrm, ref[2])
    with pytest.raises(RuntimeError, match="ema_decay"):
        _trainer(torch, encoding).extract_mesh(n, iso=iso, weights="ema")


def test_trainer_refuses_a_model_without_a_fused_kernel(gpu):
    from rtx_nerf_amd import _lib
    from rtx_nerf_amd.train import Trainer
    B = 64
    odd = Trainer(16, None, encoding="hash", n_neurons=64, n_hidden_layers=4, batch_rays=B, max_segments=B * 40,
                  hashgrid=dict(n_levels=5, n_features=2, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.5))
    with pytest.raises(_lib.RtxnError, match=r"no fused inference kernel for this model .*update_occupancy\(\)"):
        odd.extract_mesh(16, iso=1.0)
