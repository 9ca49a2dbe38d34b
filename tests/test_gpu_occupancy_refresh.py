"""rtxn_occupancy_refresh on the device (include/rtxn.h, "occupancy refresh from the live model").

The reference everywhere is a numpy float32 restatement, below, of the arithmetic the header states -- cell points, per-run
jitter, the fold, the threshold, the hierarchy -- fed with sigma obtained by calling the segment entries (tested on their own
in test_gpu_hashmlp.py / test_gpu_layer0_direction.py) on the numpy-built pseudo-segments.  Densities and bits are compared bit for bit."""
import numpy as np
import pytest

from rtx_nerf_amd import scenes

pytestmark = pytest.mark.gpu

F = np.float32
HG = (8, 2, 14, 8, 1.6)          # the suite's small hash grid: 8 levels x 2 features, 2^14 entries, base 8, growth 1.6


# ------------------------------------------------------------------------------------------------ the header, in numpy
def fmix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def run_index(R):
    nk = (R + 31) // 32
    g = np.arange(R * R * nk, dtype=np.int64)
    k, row = g % nk, g // nk
    return g, row // R, row % R, k, nk


def ref_segments(R, jitter=False, seed=0, step=0):
    """start, end float32[runs][3]: h = 2/R; p = (i + 0.5) * h - 1; + (u - 0.5) * h per run and axis; end_z = start_z + 32 h."""
    g, x, y, k, nk = run_index(R)
    h = F(2.0) / F(R)
    p = [(c.astype(F) + F(0.5)) * h - F(1.0) for c in (x, y, 32 * k)]
    if jitter:
        with np.errstate(over="ignore"):
            h0 = fmix32(np.uint32(seed) + np.uint32(0x9E3779B9) * np.uint32(step))
            for c in range(3):
                bits = fmix32(h0 ^ (np.uint32(3) * g.astype(np.uint32) + np.uint32(c))) >> np.uint32(8)
                u = bits.astype(F) * F(2.0 ** -24)
                p[c] = p[c] + (u - F(0.5)) * h
    start = np.stack(p, axis=1).astype(F)
    end = start.copy()
    end[:, 2] = start[:, 2] + F(32.0) * h
    return start, end


def ref_fold(R, density, sigma, decay, thick):
    """density[c] = v > d ? v : d with v = sigma * thick (NaN sigma = 0), d = density * decay; the in-grid cells of each run."""
    g, x, y, k, nk = run_index(R)
    z = 32 * k[:, None] + np.arange(32)[None, :]
    ok = z < R
    cell = ((x * R + y)[:, None] * R + z)[ok]
    s = sigma.astype(F)[ok]
    s = np.where(np.isnan(s), F(0), s)
    v = s * F(thick)
    d = density[cell] * F(decay)
    out = density.copy()
    out[cell] = np.where(v > d, v, d)
    return out


def pack_bits(flags):
    flat = np.ascontiguousarray(flags, dtype=bool).reshape(-1)
    b = np.packbits(flat, bitorder="little")
    b = np.concatenate([b, np.zeros((-b.size) % 4, np.uint8)])
    return b.view(np.uint32)


def ref_hierarchy(density, thr, R):
    on = (density > F(thr)).reshape(R, R, R)
    out = {"occ": pack_bits(on), "occupied": int(on.sum()), "coarse": None, "bricks": None, "super_mip": None}
    if R % 4 == 0:
        Rc = R // 4
        blk = on.reshape(Rc, 4, Rc, 4, Rc, 4).transpose(0, 2, 4, 1, 3, 5).reshape(Rc, Rc, Rc, 64)     # [X,Y,Z][dx<<4|dy<<2|dz]
        coarse = blk.any(axis=3)
        out["coarse"] = pack_bits(coarse)
        out["bricks"] = (blk.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64).reshape(-1)
        if R % 16 == 0:
            Rs = Rc // 4
            out["super_mip"] = pack_bits(coarse.reshape(Rs, 4, Rs, 4, Rs, 4).any(axis=(1, 3, 5)))
    return out


# ------------------------------------------------------------------------------------------------ models and the call
class Model:
    def __init__(self, torch, kind, seed=3, gain=1.5):
        from rtx_nerf_amd import api
        self.torch, self.api, self.kind = torch, api, kind
        rng = np.random.default_rng(seed)
        if kind == "hash":
            self.hg = api.HashGrid(*HG, n_dir_freqs=4)
            E = self.hg.encoded_width()
            self.net = api.Network(n_neurons=64, n_hidden_layers=4, n_encoded_features=E)
            # weights x gain per layer: sigma spreads over (0, 1) -- 1.5: the middle half of it, 2.5: two decades
            self.params = torch.from_numpy(scenes.xavier_params_fp16(64, 4, E, seed=seed) * np.float16(gain)).cuda()
            self.table = torch.from_numpy(rng.uniform(-0.5, 0.5, self.hg.n_params()).astype(np.float16)).cuda()
            self.first = self.table.clone()
        else:
            self.hg, self.table = None, None
            self.net = api.Network(n_neurons=128, n_hidden_layers=8)
            self.params = torch.from_numpy(scenes.xavier_params_fp16(128, 8, self.net.encoded_width(), seed=seed)).cuda()
            self.first = self.params.clone()
        self.net.set_params(self.params)

    def set_state(self, it):
        """state 0: as built; state it > 0: seeded noise in place of the table (hash) / over the weights (frequency), in place"""
        torch = self.torch
        rng = np.random.default_rng(100 + it)
        if self.kind == "hash":
            self.table.copy_(self.first if it == 0 else
                             torch.from_numpy(rng.uniform(-0.5, 0.5, self.table.numel()).astype(np.float16)).cuda())
        else:
            self.params.copy_(self.first)
            if it:
                self.params.mul_(torch.from_numpy(rng.uniform(0.7, 1.3, self.params.numel()).astype(np.float16)).cuda())
            self.net.set_params(self.params)

    def sigma(self, start, end):
        """sigma float32[runs][32] of the pseudo-segments through the segment entry the refresh itself uses"""
        torch, api = self.torch, self.api
        P = start.shape[0]
        sp, ep = torch.from_numpy(start).cuda(), torch.from_numpy(end).cuda()
        sv = torch.zeros((P, 2), device="cuda")
        total = torch.tensor([P], dtype=torch.int32, device="cuda")
        rad = torch.empty((P * 32, 4), dtype=torch.float16, device="cuda")
        if self.kind == "hash":
            api.hashmlp_forward_segments(self.net, self.hg, self.table, sp, ep, sv, total, P, rad, api.SAMPLING_REGULAR)
        else:
            self.net.forward_segments_compact(sp, ep, sv, total, P, rad)
        return rad[:, 3].float().cpu().numpy().reshape(P, 32)


class Grid:
    """the caller's buffers of one refresh target"""

    def __init__(self, torch, R, fill=0):
        z = lambda n, dt: torch.full((n,), fill, dtype=dt, device="cuda")
        self.R = R
        self.density = torch.zeros(R ** 3, device="cuda")
        self.occ = z((R ** 3 + 31) // 32, torch.int32)
        self.coarse = z(((R // 4) ** 3 + 31) // 32, torch.int32) if R % 4 == 0 else None
        self.bricks = z((R // 4) ** 3, torch.int64) if R % 4 == 0 else None
        self.super_mip = z(((R // 16) ** 3 + 31) // 32, torch.int32) if R % 16 == 0 else None
        self.occupied = z(1, torch.int32)
        self.mean = torch.zeros(1, device="cuda")
        self.ws = {}

    def refresh(self, m, *, decay, thick, threshold, mode, jitter=False, seed=0, step=None, runs_per_pass=None):
        api = m.api
        P = runs_per_pass or api.occupancy_refresh_runs(self.R)
        if P not in self.ws:
            self.ws[P] = api.occupancy_refresh_workspace(self.R, P)
        api.occupancy_refresh(m.net, grid=m.hg, table=m.table, grid_res=self.R, density=self.density, decay=decay,
                              thickness_scale=thick, threshold=threshold, threshold_mode=mode, jitter=jitter, seed=seed, step=step,
                              occupancy=self.occ, coarse=self.coarse, bricks=self.bricks, super_mip=self.super_mip,
                              occupied=self.occupied, mean=self.mean, workspace=self.ws[P], runs_per_pass=P)

    def host(self):
        u = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)
        return {"density": self.density.cpu().numpy(), "occ": u(self.occ, np.uint32), "coarse": u(self.coarse, np.uint32),
                "bricks": u(self.bricks, np.uint64), "super_mip": u(self.super_mip, np.uint32),
                "occupied": int(self.occupied.item()), "mean": self.mean.cpu().numpy().copy()}


def assert_hierarchy(got, want):
    for key in ("occ", "coarse", "bricks", "super_mip"):
        if want[key] is None:
            assert got[key] is None, key
        else:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert got["occupied"] == want["occupied"]


def assert_same_outputs(a, b):
    for key in a:
        if a[key] is None:
            assert b[key] is None
        elif key == "occupied":
            assert a[key] == b[key]
        else:
            np.testing.assert_array_equal(np.asarray(a[key]).view(np.uint8), np.asarray(b[key]).view(np.uint8), err_msg=key)


@pytest.fixture(scope="module")
def models(gpu):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = Model(gpu, kind)
        return cache[kind]
    return get


# ------------------------------------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("kind,R", [("hash", 32), ("hash", 48), ("hash", 20), ("hash", 6), ("freq", 32), ("freq", 20)])
def test_absolute_threshold_without_jitter_is_bit_exact(gpu, models, kind, R):
    """R = 32: one run per row; 48: a tail run, words straddling rows, all three mips; 20: no 16^3 mip; 6: no mip at all and
    most of every run outside the grid.  decay 0 over a zeroed density: a plain point sample at the cell centres."""
    torch = gpu
    m = models(kind)
    api = m.api
    thick = 37.0 * 2.0 / R
    start, end = ref_segments(R)
    want_density = ref_fold(R, np.zeros(R ** 3, F), m.sigma(start, end), 0.0, thick)
    thr = float(np.median(want_density))             # both bit values in quantity
    want = ref_hierarchy(want_density, thr, R)
    assert 0.1 < want["occupied"] / R ** 3 <= 0.5
    grid = Grid(torch, R, fill=0x5A5A5A5A)           # stale contents everywhere, tail words included
    grid.refresh(m, decay=0.0, thick=thick, threshold=thr, mode=api.OCC_ABSOLUTE)
    got = grid.host()
    np.testing.assert_array_equal(got["density"].view(np.uint32), want_density.view(np.uint32))
    assert_hierarchy(got, want)
    # ... and the hierarchy is what the existing builders make of the fine bits
    if R % 4 == 0:
        assert torch.equal(grid.coarse, api.build_occupancy_mip(grid.occ, R))
        assert torch.equal(grid.bricks, api.build_occupancy_bricks(grid.occ, R))
    if R % 16 == 0:
        assert torch.equal(grid.super_mip, api.build_occupancy_mip(grid.coarse, R // 4))
    assert torch.equal(grid.occ, api.occupancy_from_density(grid.density, thr, R))


# ------------------------------------------------------------------------------------------------ 2. running maximum
@pytest.mark.parametrize("kind", ["hash", "freq"])
def test_decaying_running_maximum(gpu, kind):
    """Three refreshes with decay 0.5, the table (hash) or the weights (frequency) replaced in between.  The hash model is
    built with sigma spread over two decades, so that cells exist whose sample is above the threshold once and far below it
    afterwards: they stay set while the decayed value is above the threshold and are released when it crosses.  (The 8x128
    frequency model's sigma stays within 0.49 .. 0.53 whatever the weights: no cell of it can hold at decay 0.5, its case checks
    the iterated densities and bits alone.)"""
    torch = gpu
    m = Model(torch, kind, seed=11, gain=2.5)        # its own model: the table / weights are changed below
    api = m.api
    R, decay = 32 if kind == "hash" else 20, 0.5
    thick = 37.0 * 2.0 / R
    start, end = ref_segments(R)
    # the reference first, for all three states: the refreshes' own samples and the iterated running maximum
    vals, dens, density = [], [], np.zeros(R ** 3, F)
    for it in range(3):
        m.set_state(it)
        sig = m.sigma(start, end)
        vals.append(ref_fold(R, np.zeros(R ** 3, F), sig, 0.0, thick))
        density = ref_fold(R, density, sig, decay, thick)
        dens.append(density)

    def hold_and_release(thr):
        fell = (vals[0] > thr) & (vals[1] <= thr) & (vals[2] <= thr)
        return fell, fell & (dens[1] > thr), fell & (dens[2] <= thr)

    # the threshold: of the deciles of the first sample, the one under which most cells hold once and are released after
    thr = max((float(t) for t in np.percentile(vals[0], range(10, 100, 10))),
              key=lambda t: min(hold_and_release(t)[1].sum(), hold_and_release(t)[2].sum()))
    fell, held, released = hold_and_release(thr)
    if kind == "hash":
        assert held.sum() >= 100 and released.sum() >= 100, "seed: too few cells show the hold / the release"
    grid, bits = Grid(torch, R), []
    for it in range(3):
        m.set_state(it)
        grid.refresh(m, decay=decay, thick=thick, threshold=thr, mode=api.OCC_ABSOLUTE)
        got = grid.host()
        np.testing.assert_array_equal(got["density"].view(np.uint32), dens[it].view(np.uint32))
        assert_hierarchy(got, ref_hierarchy(dens[it], thr, R))
        bits.append(np.unpackbits(got["occ"].view(np.uint8), bitorder="little")[:R ** 3].astype(bool))
    assert bits[0][fell].all() and bits[1][held].all() and not bits[1][fell & ~held].any() and not bits[2][released].any()
    assert bits[2][fell & ~released].all()


# ------------------------------------------------------------------------------------------------ 3. jitter
def test_jitter_per_run_seed_and_step(gpu, models):
    torch = gpu
    m = models("hash")
    api = m.api
    R = 32
    thick, h = 37.0 * 2.0 / R, 2.0 / R
    g, x, y, k, nk = run_index(R)
    seen, starts = {}, {}
    for seed in (7, 0xDEADBEEF):
        for step in (0, 12345):
            start, end = ref_segments(R, True, seed, step)
            # every sample point lies inside its own cell: start + (i/32)(end - start), coordinates of magnitude <= 1 formed by
            # a handful of float32 roundings (2^-24 each): 2^-21 of slack at the cell faces
            lo = np.stack([x, y, 32 * k], axis=1) * h - 1.0
            off = start.astype(np.float64) - lo
            assert (off >= -2.0 ** -21).all() and (off <= h + 2.0 ** -21).all()
            dz = end[:, 2].astype(np.float64) - start[:, 2]
            assert np.abs(dz - 32 * h).max() <= 2.0 ** -21 and (end[:, :2] == start[:, :2]).all()
            assert np.abs((off / h).mean(axis=0) - 0.5).max() < 0.05            # 1024 draws per axis: sd 0.009
            want = ref_fold(R, np.zeros(R ** 3, F), m.sigma(start, end), 0.0, thick)
            grid = Grid(torch, R)
            dstep = torch.tensor([step], dtype=torch.int32, device="cuda")
            grid.refresh(m, decay=0.0, thick=thick, threshold=1.0, mode=api.OCC_ABSOLUTE, jitter=True, seed=seed, step=dstep)
            got = grid.host()["density"]
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
            seen[(seed, step)], starts[(seed, step)] = got, start
            if step == 0:
                null = Grid(torch, R)
                null.refresh(m, decay=0.0, thick=thick, threshold=1.0, mode=api.OCC_ABSOLUTE, jitter=True, seed=seed, step=None)
                np.testing.assert_array_equal(null.host()["density"].view(np.uint32), got.view(np.uint32))
    keys = list(seen)
    for i in range(len(keys)):
        for j in range(i):
            assert (starts[keys[i]] != starts[keys[j]]).mean() > 0.99            # other offsets ...
            assert (seen[keys[i]] != seen[keys[j]]).mean() > 0.5                  # ... other samples
    centre = Grid(torch, R)
    centre.refresh(m, decay=0.0, thick=thick, threshold=1.0, mode=api.OCC_ABSOLUTE, jitter=False)
    assert (centre.host()["density"] != seen[keys[0]]).mean() > 0.5


# ------------------------------------------------------------------------------------------------ 4. passes
def test_pass_size_does_not_change_a_bit(gpu, models):
    torch = gpu
    m = models("hash")
    api = m.api
    R = 48
    thick = 37.0 * 2.0 / R
    outs = []
    for P in (1, 7, None):
        grid = Grid(torch, R)
        for it in range(2):            # the second refresh folds into a non-trivial density
            grid.refresh(m, decay=0.7, thick=thick, threshold=1e9, mode=api.OCC_MIN_MEAN, jitter=True, seed=5,
                         step=torch.tensor([it], dtype=torch.int32, device="cuda"), runs_per_pass=P)
        outs.append(grid.host())
    assert 0 < outs[0]["occupied"] < R ** 3
    assert_same_outputs(outs[0], outs[1])
    assert_same_outputs(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ 5. min(threshold, mean)
@pytest.mark.parametrize("R,threshold", [(48, 1e9), (32, 1e9), (20, 0.25)])
def test_min_mean_threshold(gpu, models, R, threshold):
    """The mean: N <= 2^17 non-negative terms summed pairwise in float and then in double -- about 20 roundings of 2^-24 on
    the way: 4e-6 relative.  The bits: density > min(threshold, mean), cells within 8e-6 thr of it left out."""
    torch = gpu
    m = models("hash")
    api = m.api
    thick = 37.0 * 2.0 / R
    start, end = ref_segments(R)
    want_density = ref_fold(R, np.zeros(R ** 3, F), m.sigma(start, end), 0.0, thick)
    mean_ref = float(want_density.astype(np.float64).mean())
    thr = min(threshold, mean_ref)
    near = np.abs(want_density.astype(np.float64) - thr) <= 8e-6 * thr
    assert near.mean() <= 0.005, "seed: too many cells on the threshold"
    assert (threshold < mean_ref) == (R == 20)       # the third case takes the given threshold, the others the mean
    outs = []
    for rep in range(2):
        grid = Grid(torch, R)
        grid.refresh(m, decay=0.0, thick=thick, threshold=threshold, mode=api.OCC_MIN_MEAN)
        outs.append(grid.host())
    got = outs[0]
    np.testing.assert_array_equal(got["density"].view(np.uint32), want_density.view(np.uint32))
    mean = float(got["mean"][0])
    assert abs(mean - float(got["density"].astype(np.float64).mean())) <= 4e-6 * mean_ref
    bits = np.unpackbits(got["occ"].view(np.uint8), bitorder="little")[:R ** 3].astype(bool)
    want_bits = want_density.astype(np.float64) > thr
    np.testing.assert_array_equal(bits[~near], want_bits[~near])
    assert abs(got["occupied"] - int(want_bits.sum())) <= int(near.sum())
    assert_same_outputs(outs[0], outs[1])             # identical state, identical call: identical bits, mean included


# ------------------------------------------------------------------------------------------------ 6. capture
def test_refresh_is_capturable(gpu, models):
    torch = gpu
    m = models("hash")
    api = m.api
    R = 32
    thick = 37.0 * 2.0 / R
    kw = dict(decay=0.5, thick=thick, threshold=1e9, mode=api.OCC_MIN_MEAN, jitter=True, seed=9)
    eager, step = Grid(torch, R), torch.tensor([40], dtype=torch.int32, device="cuda")
    want = []
    for _ in range(2):
        eager.refresh(m, step=step, **kw)
        step.add_(1)
        want.append(eager.host())
    grid, gstep = Grid(torch, R), torch.tensor([40], dtype=torch.int32, device="cuda")
    grid.refresh(m, step=gstep, **kw)                  # allocates the workspace outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grid.refresh(m, step=gstep, **kw)
        gstep.add_(1)
    grid.density.zero_()
    gstep.fill_(40)
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert_same_outputs(grid.host(), want[i])
    assert int(gstep.item()) == 42
    assert not np.array_equal(want[0]["density"], want[1]["density"])


# ------------------------------------------------------------------------------------------------ 7. Trainer
HGD = dict(n_levels=8, n_features=2, log2_hashmap_size=13, base_resolution=8, per_level_scale=1.5)


def _sphere_occ(torch, R, radius=0.72):
    return torch.from_numpy(scenes.pack_occupancy(scenes.sphere_density(R, radius)).view(np.int32).copy()).cuda()


def _hash_trainer(torch, R, occ, B):
    from rtx_nerf_amd.train import Trainer
    return Trainer(R, occ, encoding="hash", n_neurons=64, n_hidden_layers=4, hashgrid=HGD, batch_rays=B, max_segments=B * 40,
                   lr=1e-2, density_scale=100.0, seed=1)


def test_trainer_refreshes_in_place_behind_captured_steps(gpu):
    torch = gpu
    from rtx_nerf_amd.train import camera_rays
    R, W, H = 32, 24, 24
    B = W * H
    tr = _hash_trainer(torch, R, _sphere_occ(torch, R), B)
    la = scenes.pose_spherical(25.0, -30.0, origin_scale=10.0)
    f = scenes.lego_focal_length(True)
    o, d = camera_rays(la, f, W, H)
    tgt = torch.full((B, 3), 0.4, device="cuda")
    for _ in range(3):
        tr.step(o, d, tgt)
    tr.capture_step(B)
    tr.graph_rays_o.copy_(o)
    tr.graph_rays_d.copy_(d)
    tr.graph_targets.copy_(tgt)
    tr.step_captured()
    pipe = tr.render_pipeline(W, H, f, max_segments=B * 40)
    pipe.set_pose(la)
    before = pipe.render().clone()
    ptrs = [t.data_ptr() for t in (tr.occ, tr.coarse, tr.bricks, tr.super_mip)]
    old_bits = tr.occ.clone()

    # a twin with the same state takes update_occupancy()'s route; the threshold sits halfway between the median thickness
    # and the next larger value that occurs (sigma is fp16: the values are a lattice, and the median itself is taken by many cells)
    twin = _hash_trainer(torch, R, _sphere_occ(torch, R), B)
    twin.table.copy_(tr.table)
    twin.params.copy_(tr.params)
    twin.net.set_params(twin.params)
    tr.refresh_occupancy(threshold=1e-3, decay=0.0, jitter=False, threshold_mode="absolute")
    levels = np.unique(tr.occ_density.cpu().numpy())
    assert levels.size >= 2, "seed: the model is constant over the grid"
    mid = min(np.searchsorted(levels, np.median(tr.occ_density.cpu().numpy())), levels.size - 2)
    thr = float(0.5 * (np.float64(levels[mid]) + np.float64(levels[mid + 1])))
    twin.update_occupancy(thr)
    assert tr.refresh_occupancy(threshold=thr, decay=0.0, jitter=False, threshold_mode="absolute") is None
    assert [t.data_ptr() for t in (tr.occ, tr.coarse, tr.bricks, tr.super_mip)] == ptrs
    loss = tr.step_captured()                          # the captured graph reads the refreshed buffers
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    dens = tr.occ_density.cpu().numpy().astype(np.float64)
    near = np.abs(dens - thr) <= 8e-6 * thr
    assert near.mean() <= 0.005
    mine = np.unpackbits(tr.occ.cpu().numpy().view(np.uint8), bitorder="little")[:R ** 3].astype(bool)
    theirs = np.unpackbits(twin.occ.cpu().numpy().view(np.uint8), bitorder="little")[:R ** 3].astype(bool)
    np.testing.assert_array_equal(mine[~near], theirs[~near])
    np.testing.assert_array_equal(mine[~near], (dens > thr)[~near])
    assert 0 < mine.sum() < R ** 3
    frac, mean = tr.occupancy_stats()
    assert frac == mine.mean() and abs(mean - dens.mean()) <= 4e-6 * dens.mean()
    # the renderer made before the refresh draws the new grid: the same frame as a pipeline built on the new bits
    after = pipe.render().clone()
    fresh = tr.render_pipeline(W, H, f, max_segments=B * 40)
    fresh.set_pose(la)
    assert torch.equal(after, fresh.render())
    assert not torch.equal(old_bits, tr.occ) and before.shape == after.shape
    # the default call: EMA, jitter from the captured steps' device counter, min(threshold, mean)
    tr.refresh_occupancy()
    tr.step_captured()
    torch.cuda.synchronize()
    assert [t.data_ptr() for t in (tr.occ, tr.coarse, tr.bricks, tr.super_mip)] == ptrs
    assert 0.0 <= tr.occupancy_stats()[0] <= 1.0


def test_trainer_frequency_model_refreshes_from_current_weights(gpu):
    torch = gpu
    from rtx_nerf_amd import _lib, api
    from rtx_nerf_amd.train import Trainer, camera_rays
    R, W, H = 20, 16, 16
    B = W * H
    tr = Trainer(R, _sphere_occ(torch, R), encoding="freq", n_neurons=64, n_hidden_layers=2, n_dir_freqs=12, batch_rays=B,
                 max_segments=B * 30, lr=3e-2, density_scale=100.0, seed=2)
    kw = dict(threshold=1e-3, decay=0.0, jitter=False, threshold_mode="absolute")
    tr.refresh_occupancy(**kw)
    first = tr.occ_density.clone()
    o, d = camera_rays(scenes.pose_spherical(25.0, -30.0, origin_scale=10.0), scenes.lego_focal_length(True), W, H)
    for _ in range(3):
        tr.step(o, d, torch.full((B, 3), 0.9, device="cuda"))
    # the raw entry without the re-pack: the inference kernels' weights are stale, and it says so
    with pytest.raises(_lib.RtxnError, match="rtxn_mlp_set_params"):
        api.occupancy_refresh(tr.net, grid_res=R, density=tr.occ_density, decay=0.0, thickness_scale=tr.density_scale * 2.0 / R,
                              threshold=1e-3, threshold_mode=api.OCC_ABSOLUTE, occupancy=tr.occ, coarse=tr.coarse, bricks=tr.bricks,
                              workspace=tr._occ_ws, runs_per_pass=api.occupancy_refresh_runs(R))
    assert torch.equal(tr.occ_density, first)          # refused before anything ran
    tr.refresh_occupancy(**kw)
    torch.cuda.synchronize()
    assert (tr.occ_density != first).float().mean() > 0.5
    # ... and they are the current weights: sigma of the cell centres through the segment entry after the same re-pack
    start, end = ref_segments(R)
    P = start.shape[0]
    rad = torch.empty((P * 32, 4), dtype=torch.float16, device="cuda")
    tr.net.forward_segments_compact(torch.from_numpy(start).cuda(), torch.from_numpy(end).cuda(), torch.zeros((P, 2), device="cuda"),
                                    torch.tensor([P], dtype=torch.int32, device="cuda"), P, rad)
    sig = rad[:, 3].float().cpu().numpy().reshape(P, 32)
    want = ref_fold(R, np.zeros(R ** 3, F), sig, 0.0, F(tr.density_scale * 2.0 / R))
    np.testing.assert_array_equal(tr.occ_density.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_trainer_without_a_grid_and_unsupported_models(gpu):
    torch = gpu
    from rtx_nerf_amd import _lib
    from rtx_nerf_amd.train import Trainer
    R, B = 16, 64
    tr = _hash_trainer(torch, R, None, B)
    tr.capture_step(B)
    tr.refresh_occupancy(threshold=1e-3)
    assert tr.occ is not None and tr.coarse is not None and tr.bricks is not None and tr.super_mip is not None
    with pytest.raises(RuntimeError, match="capture_step"):       # its graphs traversed a dense grid: dropped, as by update_occupancy()
        tr.step_captured()
    frac, mean = tr.occupancy_stats()
    assert 0.0 <= frac <= 1.0 and mean >= 0.0
    odd = Trainer(R, None, encoding="hash", n_neurons=64, n_hidden_layers=4, batch_rays=B, max_segments=B * 40,
                  hashgrid=dict(n_levels=5, n_features=2, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.5))
    with pytest.raises(_lib.RtxnError, match=r"update_occupancy\(\)"):
        odd.refresh_occupancy()
    with pytest.raises(RuntimeError):
        odd.occupancy_stats()
