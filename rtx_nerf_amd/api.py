"""Host-side mirror of the reference's operator interface over the C ABI.

Function names, argument order and argument meaning follow the reference
headers (sampler/sampler.h:19-30, vol_render/vol_render.h:5-25,
rtx/include/params.h:14-42, and the tiny-cuda-nn calls of main.cu:325-349,721)
so the parity tests read like the reference's call sites.  Arguments are torch
CUDA tensors (plumbing: device memory + streams); all work is enqueued on
torch's current stream.  Nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import MlpConfig, TraceParams, check

NUM_SAMPLES_PER_SEGMENT = 32           # sampler/sampler.h:4
SAMPLING_REGULAR = 0                   # sampler/sampler.h:5-9
SAMPLING_STRATIFIED_JITTERING = 1
SAMPLING_UNIFORM = 2
SAMPLING_MIDPOINT_WORLD = 3               # this build: midpoints + world step lengths (for VR_NERF)
SAMPLING_JITTER_WORLD = 4                 # this build: MIDPOINT_WORLD with a per-step offset inside each stratum (sample_jitter())
TRACE_COMPAT, TRACE_DDA = 0, 1
VR_COMPAT, VR_NERF = 0, 1
ACT_NONE, ACT_SIGMOID = 0, 1


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, dtype=None, name="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.RtxnError(f"{name} must be a CUDA tensor (librtxn has no CPU path)")
    if not t.is_contiguous():
        raise _lib.RtxnError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise _lib.RtxnError(f"{name} must be {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------- traversal
def trace_grid(look_at=None, focal_length=1.0, aspect_ratio=1.0, width=0, height=0, *, grid_res,
               rays_o=None, rays_d=None, ray_begin=0, ray_count=None, occupancy=None,
               occupancy_coarse=None, occupancy_bricks=None, occupancy_super=None, mode=TRACE_COMPAT, ray_origins=None, viewing_direction=None,
               num_hits=None, intersection_arr_size=0, indices=None, start_points=None,
               end_points=None, t_start=None, t_end=None, seg_ray=None, seg_view=None, seg_first=None, num_stored=None, segment_capacity=0,
               window_chunk=0, window_stride=0, sub_rays=0, sub_hits=None):
    """optixLaunch(pipeline_ray_march, ..., width, height, 1) with Params (main.cu:481-508)."""
    p = trace_params(**{k: v for k, v in locals().items()})
    check(_lib.lib().rtxn_trace_grid(C.byref(p), _stream()), "rtxn_trace_grid")


def trace_params(look_at=None, focal_length=1.0, aspect_ratio=1.0, width=0, height=0, *, grid_res,
                 rays_o=None, rays_d=None, ray_begin=0, ray_count=None, occupancy=None,
                 occupancy_coarse=None, occupancy_bricks=None, occupancy_super=None, mode=TRACE_COMPAT, ray_origins=None, viewing_direction=None,
                 num_hits=None, intersection_arr_size=0, indices=None, start_points=None,
                 end_points=None, t_start=None, t_end=None, seg_ray=None, seg_view=None, seg_first=None, num_stored=None, segment_capacity=0,
                 window_chunk=0, window_stride=0, sub_rays=0, sub_hits=None):
    """struct rtxn_trace_params over the given tensors (which the caller keeps alive)."""
    p = TraceParams()
    p.look_at = _ptr(look_at, torch.float32, "look_at")
    p.focal_length, p.aspect_ratio = focal_length, aspect_ratio
    p.width, p.height = width, height
    p.rays_o = _ptr(rays_o, torch.float32, "rays_o")
    p.rays_d = _ptr(rays_d, torch.float32, "rays_d")
    if look_at is None and rays_o is not None and width == 0:
        p.width, p.height = rays_o.shape[0], 1
    p.ray_begin = ray_begin
    p.ray_count = (p.width * p.height - ray_begin) if ray_count is None else ray_count
    p.grid_res = grid_res
    p.occupancy = _ptr(occupancy, torch.int32, "occupancy")
    p.occupancy_coarse = _ptr(occupancy_coarse, torch.int32, "occupancy_coarse")
    p.occupancy_bricks = _ptr(occupancy_bricks, torch.int64, "occupancy_bricks")
    p.occupancy_super = _ptr(occupancy_super, torch.int32, "occupancy_super")
    p.mode = mode
    p.ray_origins = _ptr(ray_origins, torch.float32, "ray_origins")
    p.viewing_direction = _ptr(viewing_direction, torch.float32, "viewing_direction")
    p.num_hits = _ptr(num_hits, torch.int32, "num_hits")
    p.intersection_arr_size = intersection_arr_size
    p.indices = _ptr(indices, torch.int32, "indices")
    p.start_points = _ptr(start_points, torch.float32, "start_points")
    p.end_points = _ptr(end_points, torch.float32, "end_points")
    p.t_start = _ptr(t_start, torch.float32, "t_start")
    p.t_end = _ptr(t_end, torch.float32, "t_end")
    p.seg_ray = _ptr(seg_ray, torch.int32, "seg_ray")
    p.seg_view = _ptr(seg_view, torch.float32, "seg_view")
    p.seg_first = _ptr(seg_first, torch.uint8, "seg_first")
    p.num_stored = _ptr(num_stored, torch.int32, "num_stored")
    p.segment_capacity = segment_capacity
    p.window_chunk, p.window_stride = window_chunk, window_stride
    p.sub_rays = sub_rays
    p.sub_hits = _ptr(sub_hits, torch.int32, "sub_hits")
    return p


def auto_sub_rays(n_rays):
    """Lanes per ray (rtxn_trace_params.sub_rays) for a launch of n_rays: measured on MI355X (tools/trace_bench.py), the
    smaller the launch the more the longest ray's walk dominates it -- 640 k rays: 2 (0.20 -> 0.15 ms), 80 k: 8 (0.18 ->
    0.07 ms), 16 k rays: 16, a 4096-ray training batch: 32."""
    import os
    if os.environ.get("RTXN_SUB_RAYS"):          # experiments (tools/trace_bench.py, tools/probe)
        return int(os.environ["RTXN_SUB_RAYS"])
    if n_rays >= 300_000:
        return 2
    if n_rays >= 120_000:
        return 4
    if n_rays >= 30_000:
        return 8
    if n_rays >= 12_000:
        return 16
    return 32          # a 4096-ray training batch: count + scan + write 81 -> 67 us; 64 lanes per ray: no further gain


def build_occupancy_mip(occupancy, grid_res):
    rc = grid_res // 4
    words = (rc ** 3 + 31) // 32
    coarse = torch.empty(words, dtype=torch.int32, device=occupancy.device)
    check(_lib.lib().rtxn_build_occupancy_mip(_ptr(occupancy, torch.int32), grid_res, _ptr(coarse), _stream()),
          "rtxn_build_occupancy_mip")
    return coarse


def build_occupancy_bricks(occupancy, grid_res):
    rc = grid_res // 4
    bricks = torch.empty(rc ** 3, dtype=torch.int64, device=occupancy.device)
    check(_lib.lib().rtxn_build_occupancy_bricks(_ptr(occupancy, torch.int32), grid_res, _ptr(bricks), _stream()),
          "rtxn_build_occupancy_bricks")
    return bricks


def occupancy_from_density(density, threshold, grid_res):
    words = (grid_res ** 3 + 31) // 32
    occ = torch.empty(words, dtype=torch.int32, device=density.device)
    check(_lib.lib().rtxn_occupancy_from_density(_ptr(density, torch.float32, "density"), threshold, grid_res, _ptr(occ),
                                                 _stream()), "rtxn_occupancy_from_density")
    return occ


OCC_ABSOLUTE, OCC_MIN_MEAN = 0, 1


def occupancy_refresh_supported(net, grid=None):
    """True if rtxn_occupancy_refresh can evaluate this model (a fused inference kernel exists for it)."""
    return bool(_lib.lib().rtxn_occupancy_refresh_supported(net._h, grid._h if grid is not None else None,
                                                            grid.n_dir_freqs if grid is not None else 0))


def occupancy_refresh_runs(grid_res):
    """Runs of 32 z-cells in a grid_res^3 grid: the runs_per_pass that shades it in one pass."""
    return grid_res * grid_res * ((grid_res + NUM_SAMPLES_PER_SEGMENT - 1) // NUM_SAMPLES_PER_SEGMENT)


def occupancy_refresh_workspace(grid_res, runs_per_pass, device="cuda"):
    """The workspace of occupancy_refresh for passes of runs_per_pass runs (rtxn_occupancy_refresh_workspace_bytes)."""
    nbytes = int(_lib.lib().rtxn_occupancy_refresh_workspace_bytes(int(grid_res), int(runs_per_pass)))
    if nbytes == 0:
        check(1, "rtxn_occupancy_refresh_workspace_bytes")
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def occupancy_refresh(net, *, grid=None, table=None, grid_res, density, decay, thickness_scale, threshold,
                      threshold_mode=OCC_MIN_MEAN, jitter=False, seed=0, step=None, occupancy, coarse=None, bricks=None,
                      super_mip=None, occupied=None, mean=None, workspace, runs_per_pass):
    """rtxn_occupancy_refresh: sigma at one (optionally jittered) point per cell from the live model -> density = max(density *
    decay, sigma * thickness_scale) -> bits, 4^3 mip, bricks and 16^3 mip rewritten in place.  One call on the current stream,
    no host read: capturable.  step: int32 device tensor hashed into the jitter (None: 0); occupied (int32[1]) and mean
    (float32[1]) are optional device outputs."""
    R, a = int(grid_res), _lib.OccupancyRefreshArgs()
    a.mlp, a.grid = net._h, (grid._h if grid is not None else None)
    a.n_dir_freqs = int(grid.n_dir_freqs) if grid is not None else 0
    a.table_fp16 = _ptr(table, torch.float16, "table")
    a.grid_res = R
    a.density = _ptr(density, torch.float32, "density")
    a.decay, a.thickness_scale, a.threshold, a.threshold_mode = float(decay), float(thickness_scale), float(threshold), int(threshold_mode)
    a.jitter, a.seed, a.step = (1 if jitter else 0), int(seed) & 0xFFFFFFFF, _ptr(step, torch.int32, "step")
    a.occupancy, a.coarse = _ptr(occupancy, torch.int32, "occupancy"), _ptr(coarse, torch.int32, "coarse")
    a.bricks, a.super_mip = _ptr(bricks, torch.int64, "bricks"), _ptr(super_mip, torch.int32, "super_mip")
    a.occupied, a.mean = _ptr(occupied, torch.int32, "occupied"), _ptr(mean, torch.float32, "mean")
    a.workspace = _ptr(workspace, None, "workspace")
    a.workspace_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    a.runs_per_pass = int(runs_per_pass)
    rc, rs = R // 4, R // 16
    for nm, t, need in (("density", density, R ** 3), ("occupancy", occupancy, (R ** 3 + 31) // 32),
                        ("coarse", coarse, (rc ** 3 + 31) // 32), ("bricks", bricks, rc ** 3), ("super_mip", super_mip, (rs ** 3 + 31) // 32),
                        ("occupied", occupied, 1), ("mean", mean, 1), ("step", step, 1)):
        if t is not None and t.numel() < need:
            raise _lib.RtxnError(f"occupancy_refresh: {nm} holds {t.numel()} elements, {need} needed for grid_res {R}")
    if grid is not None and table is not None and table.numel() < grid.n_params():
        raise _lib.RtxnError(f"occupancy_refresh: table holds {table.numel()} parameters, the grid has {grid.n_params()}")
    check(_lib.lib().rtxn_occupancy_refresh(C.byref(a), _stream()), "rtxn_occupancy_refresh")


# --------------------------------------------------------------------------- mesh extraction
def _box(who, aabb):
    try:
        lo, hi = [tuple(float(v) for v in b) for b in aabb]
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError
    except (TypeError, ValueError):
        raise _lib.RtxnError(f"{who}: aabb = {aabb!r}: ((lo_x, lo_y, lo_z), (hi_x, hi_y, hi_z))") from None
    return lo, hi


def density_lattice_runs(n):
    """Runs of 32 z-nodes in a lattice of n = (n_x, n_y, n_z) nodes: the runs_per_pass that shades it in one pass."""
    return n[0] * n[1] * ((n[2] + NUM_SAMPLES_PER_SEGMENT - 1) // NUM_SAMPLES_PER_SEGMENT)


def density_lattice_workspace(n, runs_per_pass, device="cuda"):
    """The workspace of density_lattice for passes of runs_per_pass runs (rtxn_density_lattice_workspace_bytes)."""
    nbytes = int(_lib.lib().rtxn_density_lattice_workspace_bytes((C.c_int * 3)(*[int(v) for v in n]), int(runs_per_pass)))
    if nbytes == 0:
        check(1, "rtxn_density_lattice_workspace_bytes")
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def density_lattice(net, *, grid=None, table=None, resolution, aabb=((-1, -1, -1), (1, 1, 1)), scale=1.0, out=None, workspace=None,
                    runs_per_pass=None):
    """rtxn_density_lattice: sigma * scale of the model at the nodes of a regular lattice over aabb = (lo, hi) inside [-1, 1]^3,
    through the fused inference kernels.  resolution: nodes per axis, an int or (n_x, n_y, n_z), each in [2, 1024].  Returns
    float32 [n_x, n_y, n_z] (`out`, or a new tensor).  runs_per_pass: runs of 32 z-nodes shaded per pass (default: the lattice
    in one pass up to 65536 runs); the result does not depend on it.  With out and workspace given the call only enqueues:
    no host read, capturable."""
    n = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(v) for v in resolution)
    if len(n) != 3:
        raise _lib.RtxnError(f"density_lattice: resolution = {resolution!r}: an int or three")
    lo, hi = _box("density_lattice", aabb)
    runs = density_lattice_runs(n)
    P = max(1, min(runs, int(runs_per_pass) if runs_per_pass else 1 << 16))
    a = _lib.DensityLatticeArgs()
    a.mlp, a.grid = net._h, (grid._h if grid is not None else None)
    a.n_dir_freqs = int(grid.n_dir_freqs) if grid is not None else 0
    a.table_fp16 = _ptr(table, torch.float16, "table")
    a.n, a.lo, a.hi, a.scale = (C.c_int * 3)(*n), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), float(scale)
    a.runs_per_pass = P
    if grid is not None and table is not None and table.numel() < grid.n_params():
        raise _lib.RtxnError(f"density_lattice: table holds {table.numel()} parameters, the grid has {grid.n_params()}")
    if out is not None and out.numel() != n[0] * n[1] * n[2]:
        raise _lib.RtxnError(f"density_lattice: out holds {out.numel()} elements, the lattice has {n[0] * n[1] * n[2]}")
    if all(2 <= v <= 1024 for v in n):                        # otherwise the library names the field
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device="cuda")
        if workspace is None:
            workspace = density_lattice_workspace(n, P, device=out.device)
    a.density = _ptr(out, torch.float32, "out")
    a.workspace = _ptr(workspace, None, "workspace")
    a.workspace_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    check(_lib.lib().rtxn_density_lattice(C.byref(a), _stream()), "rtxn_density_lattice")
    return out.view(n)


def isosurface_workspace(n, device="cuda"):
    """The workspace of isosurface for a lattice of n = (n_x, n_y, n_z) nodes (rtxn_isosurface_workspace_bytes)."""
    nbytes = int(_lib.lib().rtxn_isosurface_workspace_bytes((C.c_int * 3)(*[int(v) for v in n])))
    if nbytes == 0:
        check(1, "rtxn_isosurface_workspace_bytes")
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def isosurface(density, iso, aabb, *, normals=True, max_vertices=None, max_triangles=None, counts=None, vertices=None, triangles=None,
               normals_out=None, workspace=None):
    """rtxn_isosurface: the indexed triangle mesh of {density > iso} by marching tetrahedra.  density: float32 [n_x, n_y, n_z]
    on the device; aabb = (lo, hi): the positions of its first and last node.  Returns (vertices float32[V, 3], triangles
    int32[T, 3], normals float32[V, 3] | None, counts int32[3] = (n_vertices, n_triangles, overflow) on the device); triangles
    wind counter-clockwise seen from the side of lower density, normals point there.
    With no capacities given the call counts first, reads the two totals on the host and allocates exactly.  With max_vertices
    and max_triangles given it only enqueues -- no host read, capturable once counts, vertices, triangles, normals_out and
    workspace are given too: the arrays come back at full capacity, entries past counts[0] / counts[1] are not written, and
    counts[2] = 1 says a capacity was too small (the totals are still the true ones)."""
    if density.dim() != 3:
        raise _lib.RtxnError(f"isosurface: density of shape {tuple(density.shape)}: [n_x, n_y, n_z]")
    n = tuple(int(v) for v in density.shape)
    lo, hi = _box("isosurface", aabb)
    dev = density.device
    if (max_vertices is None) != (max_triangles is None):
        raise _lib.RtxnError("isosurface: give both max_vertices and max_triangles, or neither")
    if workspace is None and all(2 <= v <= 1024 for v in n):
        workspace = isosurface_workspace(n, device=dev)
    if counts is None:
        counts = torch.empty(3, dtype=torch.int32, device=dev)
    a = _lib.IsosurfaceArgs()
    a.density = _ptr(density, torch.float32, "density")
    a.n, a.lo, a.hi, a.iso = (C.c_int * 3)(*n), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), float(iso)
    a.counts = _ptr(counts, torch.int32, "counts")
    a.workspace = _ptr(workspace, None, "workspace")
    a.workspace_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    if counts.numel() < 3:
        raise _lib.RtxnError(f"isosurface: counts holds {counts.numel()} elements, 3 needed")
    if max_vertices is None:
        check(_lib.lib().rtxn_isosurface(C.byref(a), _stream()), "rtxn_isosurface")        # vertices == triangles == NULL: counts only
        max_vertices, max_triangles = (int(v) for v in counts[:2].tolist())
        vertices = triangles = normals_out = None
    max_vertices, max_triangles = int(max_vertices), int(max_triangles)
    if vertices is None:
        vertices = torch.empty((max(max_vertices, 0), 3), dtype=torch.float32, device=dev)
    if triangles is None:
        triangles = torch.empty((max(max_triangles, 0), 3), dtype=torch.int32, device=dev)
    if normals and normals_out is None:
        normals_out = torch.empty((max(max_vertices, 0), 3), dtype=torch.float32, device=dev)
    if not normals:
        normals_out = None
    for nm, t, need in (("vertices", vertices, 3 * max_vertices), ("normals_out", normals_out, 3 * max_vertices),
                        ("triangles", triangles, 3 * max_triangles)):
        if t is not None and t.numel() < need:
            raise _lib.RtxnError(f"isosurface: {nm} holds {t.numel()} elements, {need} needed")
    a.vertices, a.normals = _ptr(vertices, torch.float32, "vertices"), _ptr(normals_out, torch.float32, "normals_out")
    a.triangles = _ptr(triangles, torch.int32, "triangles")
    a.max_vertices, a.max_triangles = max_vertices, max_triangles
    check(_lib.lib().rtxn_isosurface(C.byref(a), _stream()), "rtxn_isosurface")
    return vertices, triangles, normals_out, counts


def write_ply(path, vertices, triangles, normals=None):
    """A binary little-endian PLY of an indexed triangle mesh: vertices [V, 3] (x y z), optional normals [V, 3] (nx ny nz) as
    float32, faces as uchar 3 + three int32.  Tensors are copied to the host; numpy arrays are taken as they are."""
    def host(t, dtype):
        return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=dtype).reshape(-1, 3)
    v, f = host(vertices, "<f4"), host(triangles, "<i4")
    cols = [v]
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        nrm = host(normals, "<f4")
        if nrm.shape != v.shape:
            raise ValueError(f"write_ply: {nrm.shape[0]} normals for {v.shape[0]} vertices")
        cols.append(nrm)
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"write_ply: a triangle names vertex {int(f.max() if f.max() >= v.shape[0] else f.min())} of {v.shape[0]}")
    faces = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"], faces["v"] = 3, f
    with open(path, "wb") as out:
        out.write((f"ply\nformat binary_little_endian 1.0\ncomment rtx_nerf_amd isosurface\nelement vertex {v.shape[0]}\n{props}"
                   f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii"))
        out.write(np.ascontiguousarray(np.concatenate(cols, axis=1)).tobytes())
        out.write(faces.tobytes())


# --------------------------------------------------------------------------- CSR compaction
def scan_hits(num_hits, indices=None, total=None, workspace=None):
    """thrust::reduce + thrust::exclusive_scan (main.cu:631-637); total stays on the device."""
    n = num_hits.numel()
    dev = num_hits.device
    if indices is None:
        indices = torch.empty(n, dtype=torch.int32, device=dev)
    if total is None:
        total = torch.empty(1, dtype=torch.int32, device=dev)
    need = _lib.lib().rtxn_scan_workspace_bytes(n)
    if workspace is None:
        workspace = torch.empty((need + 3) // 4, dtype=torch.int32, device=dev)
    check(_lib.lib().rtxn_scan_hits(_ptr(num_hits, torch.int32, "num_hits"), _ptr(indices, torch.int32),
                                    _ptr(total, torch.int32), n, _ptr(workspace), workspace.numel() * 4, _stream()),
          "rtxn_scan_hits")
    return indices, total


# --------------------------------------------------------------------------- sampler
def sample_jitter(seed=0, step=None):
    """struct rtxn_sample_jitter (include/rtxn.h) for SAMPLING_JITTER_WORLD: the offsets are hashed from `seed`, the device int32
    tensor `step` (None: 0, or opt.step for train_step) and the sample's index.  The tensor must outlive the calls."""
    j = _lib.SampleJitter()
    j.seed = int(seed) & 0xFFFFFFFF
    j.step = _ptr(step, torch.int32, "step")
    return j


def _jit(jitter):
    return C.byref(jitter) if jitter is not None else None


def launchSampler(d_start_points, d_end_points, d_view_dirs, d_t_vals, d_sampled_points, batch_size,
                  grid_res, d_num_hits, d_indices, sample_type=SAMPLING_REGULAR, jitter=None):
    """sampler/sampler.h:19-30 (the stream argument is torch's current stream).  jitter: sample_jitter(...) -> rtxn_sample_ex."""
    if jitter is not None:
        check(_lib.lib().rtxn_sample_ex(_ptr(d_start_points, torch.float32, "d_start_points"),
                                        _ptr(d_end_points, torch.float32, "d_end_points"),
                                        _ptr(d_view_dirs, torch.float32, "d_view_dirs"),
                                        _ptr(d_t_vals, torch.float32, "d_t_vals"),
                                        _ptr(d_sampled_points, torch.float32, "d_sampled_points"),
                                        batch_size, grid_res, _ptr(d_num_hits, torch.int32, "d_num_hits"),
                                        _ptr(d_indices, torch.int32, "d_indices"), sample_type, _jit(jitter), _stream()),
              "rtxn_sample_ex")
        return
    check(_lib.lib().rtxn_sample(_ptr(d_start_points, torch.float32, "d_start_points"),
                                 _ptr(d_end_points, torch.float32, "d_end_points"),
                                 _ptr(d_view_dirs, torch.float32, "d_view_dirs"),
                                 _ptr(d_t_vals, torch.float32, "d_t_vals"),
                                 _ptr(d_sampled_points, torch.float32, "d_sampled_points"),
                                 batch_size, grid_res, _ptr(d_num_hits, torch.int32, "d_num_hits"),
                                 _ptr(d_indices, torch.int32, "d_indices"), sample_type, _stream()),
          "rtxn_sample")


# --------------------------------------------------------------------------- volume rendering
def launch_volrender_cuda(network_inputs, network_outputs, num_hits, indices, ray_hit, batch_size,
                          num_samples_per_hit, pixels, mode=VR_COMPAT):
    """vol_render/vol_render.h:5-13."""
    check(_lib.lib().rtxn_volrender_fwd(_ptr(network_inputs), _ptr(network_outputs, torch.float32, "network_outputs"),
                                        _ptr(num_hits, torch.int32, "num_hits"), _ptr(indices, torch.int32, "indices"),
                                        _ptr(ray_hit, torch.float32, "ray_hit"), batch_size, num_samples_per_hit,
                                        _ptr(pixels, torch.float32, "pixels"), mode, _stream()),
          "rtxn_volrender_fwd")


def launch_volrender_backward_cuda(loss_values, loss_gradients, sampled_points_radiance, t_hit, num_hits,
                                   indices, batch_size, num_samples_per_hit, radiance_gradients, mode=VR_COMPAT):
    """vol_render/vol_render.h:15-25."""
    check(_lib.lib().rtxn_volrender_bwd(_ptr(loss_values), _ptr(loss_gradients, torch.float16, "loss_gradients"),
                                        _ptr(sampled_points_radiance, torch.float32, "sampled_points_radiance"),
                                        _ptr(t_hit, torch.float32, "t_hit"), _ptr(num_hits, torch.int32, "num_hits"),
                                        _ptr(indices, torch.int32, "indices"), batch_size, num_samples_per_hit,
                                        _ptr(radiance_gradients, torch.float16, "radiance_gradients"), mode, _stream()),
          "rtxn_volrender_bwd")


def _byref(s):
    return C.byref(s) if s is not None else None


def _composite_train(who, args, structs):
    """rtxn_<who>: the twelve arguments every training-compositor entry point begins with (`args`, in the order of
    volrender_l2_train's), then the entry point's own structs (`structs`: background, loss, regularizer, scaler, as far as it
    has them).  The loss's opacity buffer and the regulariser's tensors are sized here; the library checks the rest."""
    (network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale, pixels, loss_gradients, loss_sum,
     radiance_gradients) = args
    loss, regularizer = (tuple(structs) + (None, None, None))[1:3]
    _check_depth(who, structs[4] if len(structs) > 4 else None, batch_size, ray_hit.numel() // int(num_samples_per_hit))
    if loss is not None and loss.opacity and loss._opacity_tensor.numel() < batch_size:
        raise _lib.RtxnError(f"{who}: opacity holds {loss._opacity_tensor.numel()} elements, {batch_size} rays")
    _check_regularizer(who, regularizer, batch_size, ray_hit.numel() // int(num_samples_per_hit))
    check(getattr(_lib.lib(), "rtxn_" + who)(
        _ptr(network_outputs, torch.float32, "network_outputs"), _ptr(ray_hit, torch.float32, "ray_hit"), _ptr(num_hits, torch.int32, "num_hits"),
        _ptr(indices, torch.int32, "indices"), batch_size, num_samples_per_hit, _ptr(target, torch.float32, "target"), loss_scale,
        _ptr(pixels, torch.float32, "pixels"), _ptr(loss_gradients, torch.float16, "loss_gradients"), _ptr(loss_sum, torch.float32, "loss_sum"),
        _ptr(radiance_gradients, torch.float16, "radiance_gradients"), *[_byref(x) for x in structs], _stream()), "rtxn_" + who)


def volrender_l2_train(network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale, pixels,
                       loss_gradients, loss_sum, radiance_gradients):
    """launch_volrender_cuda + L2 loss->evaluate + launch_volrender_backward_cuda (main.cu:737-767) in one launch (VR_NERF)."""
    _composite_train("volrender_l2_train", (network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale,
                                            pixels, loss_gradients, loss_sum, radiance_gradients), ())


BG_NONE, BG_CONSTANT, BG_RANDOM = 0, 1, 2   # enum rtxn_train_background_mode


def train_background(background=None, *, seed=0, step=None, target_channels=3):
    """struct rtxn_train_background (include/rtxn.h) or None: background None (mode NONE), three floats (CONSTANT) or "random"
    (RANDOM: hashed from `seed` and the device int32 tensor `step` -- None: 0, or opt.step for train_step).  target_channels:
    3, or 4 for straight RGBA targets composited over the ray's background in the kernel.  The tensor must outlive the calls."""
    b = _lib.TrainBackground()
    b.target_channels = int(target_channels)
    if background is None:
        b.mode = BG_NONE
    elif isinstance(background, str):
        if background != "random":
            raise ValueError(f"background {background!r}: None, (r, g, b) or 'random'")
        b.mode = BG_RANDOM
    else:
        vals = [float(v) for v in background]
        if len(vals) != 3:
            raise ValueError(f"background {background!r}: three floats")
        b.mode = BG_CONSTANT
        b.color[:] = vals
    b.seed = int(seed) & 0xFFFFFFFF
    b.step = _ptr(step, torch.int32, "step")
    return b


def volrender_l2_train_ex(network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale, pixels,
                          loss_gradients, loss_sum, radiance_gradients, background):
    """volrender_l2_train over a background (background: train_background(...) or None = the plain call): pixel = sum w c +
    (1 - A) bg, fitted to the (composited) target; exact gradients of that pixel."""
    _composite_train("volrender_l2_train_ex", (network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale,
                                               pixels, loss_gradients, loss_sum, radiance_gradients), (background,))


LOSS_L2, LOSS_L1, LOSS_HUBER, LOSS_RELATIVE_L2 = 0, 1, 2, 3   # enum rtxn_loss_kind
LOSS_KINDS = {"l2": LOSS_L2, "l1": LOSS_L1, "huber": LOSS_HUBER, "relative_l2": LOSS_RELATIVE_L2}
LOSS_DEFAULT_PARAM = {LOSS_HUBER: 0.1, LOSS_RELATIVE_L2: 1e-2}      # delta (instant-ngp's); epsilon (tiny-cuda-nn's)


def train_loss(kind="l2", param=None, opacity_weight=0.0, opacity=None):
    """struct rtxn_train_loss (include/rtxn.h): kind "l2" | "l1" | "huber" | "relative_l2"; param: Huber's delta (default 0.1) or
    relative L2's epsilon (default 1e-2); opacity_weight: lambda of the alpha term lambda (A - alpha)^2 (needs RGBA targets);
    opacity: optional device float32[n_rays] the compositor writes every ray's A into (kept referenced by the struct)."""
    if kind not in LOSS_KINDS:
        raise ValueError(f"loss {kind!r}: one of {sorted(LOSS_KINDS)}")
    s = _lib.TrainLoss()
    s.kind = LOSS_KINDS[kind]
    s.param = float(param) if param is not None else LOSS_DEFAULT_PARAM.get(s.kind, 0.0)
    s.opacity_weight = float(opacity_weight)
    s.opacity = _ptr(opacity, torch.float32, "opacity")
    s._opacity_tensor = opacity
    return s


def volrender_loss_train(network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale, pixels,
                         loss_gradients, loss_sum, radiance_gradients, background=None, loss=None):
    """volrender_l2_train_ex with the loss of train_loss(...) (None, or plain "l2": that very call): the loss compositor."""
    _composite_train("volrender_loss_train", (network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale,
                                              pixels, loss_gradients, loss_sum, radiance_gradients), (background, loss))


def train_regularizer(distortion_weight=0.0, t_start=None, t_end=None, distortion=None, depth=None):
    """struct rtxn_train_regularizer (include/rtxn.h): the distortion regulariser of mip-NeRF 360 in the training compositor.
    distortion_weight: lambda_d >= 0, for world distances (a lambda quoted for distances normalised to [0, 1] is divided by the
    cube's diagonal 2 sqrt(3)); t_start, t_end: device float32 per packed segment slot, as trace_grid writes them (TRACE_DDA);
    distortion, depth: optional device float32[n_rays] outputs, L_r and sum w m of every ray.  The tensors stay referenced by the
    struct."""
    s = _lib.TrainRegularizer()
    s.distortion_weight = float(distortion_weight)
    s.t_start, s.t_end = _ptr(t_start, torch.float32, "t_start"), _ptr(t_end, torch.float32, "t_end")
    s.distortion, s.depth = _ptr(distortion, torch.float32, "distortion"), _ptr(depth, torch.float32, "depth")
    s._tensors = {"t_start": t_start, "t_end": t_end, "distortion": distortion, "depth": depth}
    return s


def _check_regularizer(who, reg, n_rays, n_segments=None):
    tensors = getattr(reg, "_tensors", None)       # a _lib.TrainRegularizer filled by hand: nothing to size, the library checks the rest
    if reg is None or tensors is None:
        return
    for nm in ("distortion", "depth"):
        t = tensors[nm]
        if t is not None and t.numel() < int(n_rays):
            raise _lib.RtxnError(f"{who}: regularizer.{nm} holds {t.numel()} elements, {n_rays} rays")
    if n_segments is not None:
        for nm in ("t_start", "t_end"):
            t = tensors[nm]
            if t is not None and t.numel() < int(n_segments):
                raise _lib.RtxnError(f"{who}: regularizer.{nm} holds {t.numel()} elements, {n_segments} segment slots")


def volrender_reg_train(network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale, pixels,
                        loss_gradients, loss_sum, radiance_gradients, background=None, loss=None, regularizer=None):
    """volrender_loss_train with the regulariser of train_regularizer(...) (None, or weight 0 without outputs: that very call)."""
    _composite_train("volrender_reg_train", (network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale,
                                             pixels, loss_gradients, loss_sum, radiance_gradients), (background, loss, regularizer))


DEPTH_LOSS_KINDS = {"l2": LOSS_L2, "l1": LOSS_L1, "huber": LOSS_HUBER}


def train_depth(weight=0.0, kind="l2", param=None, target=None, t_start=None, t_end=None, depth=None, depth_loss=None):
    """struct rtxn_train_depth (include/rtxn.h): depth supervision in the training compositor, (lambda_z / n_rays) sum_r l(D_r - z_r)
    over the rays with a target z_r > 0, D_r = sum w m.  weight: lambda_z >= 0; kind "l2" | "l1" | "huber", param: Huber's delta
    (default 0.1); target: device float32[n_rays], distances along the ray in world units (depth_targets() writes them; 0: no
    target); t_start, t_end: as train_regularizer's (the same tensors when both are given); depth, depth_loss: optional device
    float32[n_rays] outputs, D_r and l(e_r) of every ray.  The tensors stay referenced by the struct."""
    if kind not in DEPTH_LOSS_KINDS:
        raise ValueError(f"depth loss {kind!r}: one of {sorted(DEPTH_LOSS_KINDS)}")
    s = _lib.TrainDepth()
    s.weight, s.kind = float(weight), DEPTH_LOSS_KINDS[kind]
    s.param = float(param) if param is not None else LOSS_DEFAULT_PARAM.get(s.kind, 0.0)
    s.target = _ptr(target, torch.float32, "target")
    s.t_start, s.t_end = _ptr(t_start, torch.float32, "t_start"), _ptr(t_end, torch.float32, "t_end")
    s.depth, s.depth_loss = _ptr(depth, torch.float32, "depth"), _ptr(depth_loss, torch.float32, "depth_loss")
    s._tensors = {"target": target, "t_start": t_start, "t_end": t_end, "depth": depth, "depth_loss": depth_loss}
    return s


def _check_depth(who, depth, n_rays, n_segments=None):
    tensors = getattr(depth, "_tensors", None)     # a _lib.TrainDepth filled by hand: nothing to size, the library checks the rest
    if depth is None or tensors is None:
        return
    for nm in ("target", "depth", "depth_loss"):
        t = tensors[nm]
        if t is not None and t.numel() < int(n_rays):
            raise _lib.RtxnError(f"{who}: depth.{nm} holds {t.numel()} elements, {n_rays} rays")
    if n_segments is not None:
        for nm in ("t_start", "t_end"):
            t = tensors[nm]
            if t is not None and t.numel() < int(n_segments):
                raise _lib.RtxnError(f"{who}: depth.{nm} holds {t.numel()} elements, {n_segments} segment slots")


def volrender_depth_train(network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale, pixels,
                          loss_gradients, loss_sum, radiance_gradients, background=None, loss=None, regularizer=None, scaler=None, depth=None):
    """volrender_reg_train / volrender_scaled_train (scaler given: loss_scale is not read) with the depth term of train_depth(...)
    (None, or weight 0 without outputs: that very call)."""
    _composite_train("volrender_depth_train", (network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target,
                                               0.0 if scaler is not None else loss_scale, pixels, loss_gradients, loss_sum, radiance_gradients),
                     (background, loss, regularizer, scaler, depth))


# --------------------------------------------------------------------------- MLP
class Network:
    """tcnn::create_from_config(n_input_dims=5, n_output_dims=4, config) (main.cu:35-69,325)."""

    def __init__(self, n_neurons=128, n_hidden_layers=8, n_pos_freqs=10, n_dir_freqs=12, n_pos_dims=3,
                 n_dir_dims=2, n_output_dims=4, output_activation=ACT_SIGMOID, n_encoded_features=0):
        """n_encoded_features > 0: the model takes pre-encoded input of that width (RTXN_ENC_EXTERNAL)."""
        self.cfg = MlpConfig(n_pos_dims, n_pos_freqs, n_dir_dims, n_dir_freqs, n_neurons, n_hidden_layers,
                             n_output_dims, output_activation, 1 if n_encoded_features else 0, n_encoded_features)
        h = C.c_void_p()
        check(_lib.lib().rtxn_mlp_create(C.byref(self.cfg), C.byref(h)), "rtxn_mlp_create")
        self._h = h
        self.params = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:   # not during interpreter shutdown
            _lib._lib.rtxn_mlp_destroy(h)

    def n_params(self):
        return int(_lib.lib().rtxn_mlp_n_params(self._h))

    def padded_output_width(self):
        return int(_lib.lib().rtxn_mlp_padded_output_width(self._h))

    def set_reserved_cus(self, n_cus):
        """Keep n_cus CUs free of the persistent inference grid (for a collective library's kernels on other streams)."""
        check(_lib.lib().rtxn_mlp_set_reserved_cus(self._h, int(n_cus)), "rtxn_mlp_set_reserved_cus")

    def encoded_width(self):
        return int(_lib.lib().rtxn_mlp_encoded_width(self._h))

    def mfma_shape(self):
        """16: the fused inference kernels (v_mfma_f32_16x16x32_f16); 0: no fused inference kernel (pre-encoded input)."""
        return int(_lib.lib().rtxn_mlp_mfma_shape(self._h))

    def flops_per_sample(self):
        w, p, nh = self.cfg.n_neurons, self.encoded_width(), self.cfg.n_hidden_layers
        return 2 * (p * w + (nh - 1) * w * w + 16 * w)

    def initialize_params(self, seed=1337):
        """network->initialize_params(rng, params_full_precision) (main.cu:344-349): host fp32."""
        out = torch.empty(self.n_params(), dtype=torch.float32)
        check(_lib.lib().rtxn_mlp_initialize_params(self._h, seed, C.c_void_p(out.data_ptr())),
              "rtxn_mlp_initialize_params")
        return out

    def set_params(self, params_fp16):
        """network->set_params(params, params_inference, gradients) (main.cu:342)."""
        if params_fp16.numel() != self.n_params():
            raise _lib.RtxnError(f"params has {params_fp16.numel()} elements, model needs {self.n_params()}")
        self.params = params_fp16
        check(_lib.lib().rtxn_mlp_set_params(self._h, _ptr(params_fp16, torch.float16, "params"), _stream()),
              "rtxn_mlp_set_params")

    def set_params_training(self, params_fp16):
        """Per-step update inside a training loop: re-packs the training kernels' weights only (set_params() again before
        rendering with the fused inference kernels)."""
        if params_fp16.numel() != self.n_params():
            raise _lib.RtxnError(f"params has {params_fp16.numel()} elements, model needs {self.n_params()}")
        self.params = params_fp16
        check(_lib.lib().rtxn_mlp_set_params_training(self._h, _ptr(params_fp16, torch.float16, "params"), _stream()),
              "rtxn_mlp_set_params_training")

    def forward(self, input_batch, output=None):
        """network->forward(stream, input(5xN), &output(16xN)) (main.cu:715-721)."""
        n = input_batch.numel() // 5
        if output is None:
            output = torch.empty((n, 16), dtype=torch.float16, device=input_batch.device)
        check(_lib.lib().rtxn_mlp_forward(self._h, _ptr(input_batch, torch.float32, "input"), _ptr(output, torch.float16),
                                          n, _stream()), "rtxn_mlp_forward")
        return output

    def forward_radiance(self, input_batch, radiance=None):
        """forward + convertHalfToFloat of rows 0..3 (main.cu:721-728)."""
        n = input_batch.numel() // 5
        if radiance is None:
            radiance = torch.empty((n, 4), dtype=torch.float32, device=input_batch.device)
        check(_lib.lib().rtxn_mlp_forward_radiance(self._h, _ptr(input_batch, torch.float32, "input"),
                                                   _ptr(radiance, torch.float32), n, _stream()),
              "rtxn_mlp_forward_radiance")
        return radiance

    def forward_segments(self, start_points, end_points, seg_view, total_segments, max_segments, radiance,
                         t_vals=None):
        """launchSampler(REGULAR) + forward + glue fused over packed segments."""
        check(_lib.lib().rtxn_mlp_forward_segments(
            self._h, _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points"),
            _ptr(seg_view, torch.float32, "seg_view"), _ptr(total_segments, torch.int32, "total_segments"),
            max_segments, _ptr(radiance, torch.float32, "radiance"), _ptr(t_vals, torch.float32, "t_vals"), _stream()),
            "rtxn_mlp_forward_segments")
        return radiance


def _net_forward_segments_compact(self, start_points, end_points, seg_view, total_segments, max_segments, radiance_half4):
    """As forward_segments, but stores the network's four half outputs per sample (half[N, 4]) and no t_vals."""
    check(_lib.lib().rtxn_mlp_forward_segments_compact(
        self._h, _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points"),
        _ptr(seg_view, torch.float32, "seg_view"), _ptr(total_segments, torch.int32, "total_segments"),
        max_segments, _ptr(radiance_half4, torch.float16, "radiance_half4"), _stream()), "rtxn_mlp_forward_segments_compact")
    return radiance_half4


Network.forward_segments_compact = _net_forward_segments_compact


def _net_ray_direction_bias_supported(self):
    """True for the models whose segment kernels have the per-ray form (64 / 128 wide, Composite-Frequency)."""
    return bool(_lib.lib().rtxn_mlp_ray_direction_bias_supported(self._h))


def _net_ray_direction_bias(self, viewing_direction, num_hits, ray_bias):
    """Layer 0's direction product of every ray that hit: ray_bias float[n_rays, n_neurons] (rtxn_mlp_ray_direction_bias)."""
    n = int(num_hits.numel())
    check(_lib.lib().rtxn_mlp_ray_direction_bias(
        self._h, _ptr(viewing_direction, torch.float32, "viewing_direction"), _ptr(num_hits, torch.int32, "num_hits"), n,
        _ptr(ray_bias, torch.float32, "ray_bias"), _stream()), "rtxn_mlp_ray_direction_bias")
    return ray_bias


def _net_forward_segments_rays(self, start_points, end_points, seg_ray, ray_bias, total_segments, max_segments, radiance,
                               t_vals=None):
    """forward_segments (float32 radiance) or forward_segments_compact (float16) with the segments' ray index and the rays'
    table of ray_direction_bias() in place of seg_view."""
    n_rays = int(ray_bias.shape[0])
    args = (self._h, _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points"),
            _ptr(seg_ray, torch.int32, "seg_ray"), _ptr(ray_bias, torch.float32, "ray_bias"), n_rays,
            _ptr(total_segments, torch.int32, "total_segments"), max_segments)
    if radiance.dtype == torch.float16:
        check(_lib.lib().rtxn_mlp_forward_segments_rays_compact(*args, _ptr(radiance, torch.float16, "radiance_half4"), _stream()),
              "rtxn_mlp_forward_segments_rays_compact")
    else:
        check(_lib.lib().rtxn_mlp_forward_segments_rays(*args, _ptr(radiance, torch.float32, "radiance"),
                                                        _ptr(t_vals, torch.float32, "t_vals"), _stream()),
              "rtxn_mlp_forward_segments_rays")
    return radiance


Network.ray_direction_bias_supported = _net_ray_direction_bias_supported
Network.ray_direction_bias = _net_ray_direction_bias
Network.forward_segments_rays = _net_forward_segments_rays


def volrender_compact(radiance_half4, num_hits, indices, batch_size, num_samples_per_hit, pixels):
    """RTXN_VR_COMPAT compositing of half[N, 4] radiance with the implicit REGULAR t_vals (i + 1) / K."""
    check(_lib.lib().rtxn_volrender_fwd_compact(_ptr(radiance_half4, torch.float16, "radiance_half4"),
                                                _ptr(num_hits, torch.int32, "num_hits"), _ptr(indices, torch.int32, "indices"),
                                                batch_size, num_samples_per_hit, _ptr(pixels, torch.float32, "pixels"), _stream()),
          "rtxn_volrender_fwd_compact")


def volrender_compact_nerf(radiance_half4, segment_step, num_hits, indices, batch_size, num_samples_per_hit, pixels):
    """RTXN_VR_NERF compositing of half[N, 4] radiance with ONE step length per segment (float[P])."""
    check(_lib.lib().rtxn_volrender_fwd_compact_nerf(_ptr(radiance_half4, torch.float16, "radiance_half4"),
                                                     _ptr(segment_step, torch.float32, "segment_step"),
                                                     _ptr(num_hits, torch.int32, "num_hits"), _ptr(indices, torch.int32, "indices"),
                                                     batch_size, num_samples_per_hit, _ptr(pixels, torch.float32, "pixels"), _stream()),
          "rtxn_volrender_fwd_compact_nerf")


RADIANCE_FLOAT4, RADIANCE_HALF4 = 0, 1   # enum rtxn_radiance_layout


def volrender_fwd_aux(radiance, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, pixels, *, mode=VR_COMPAT,
                      sample_type=SAMPLING_REGULAR, t_start=None, t_end=None, depth=None, opacity=None, background=None):
    """Colour, opacity (sum of the weights) and expected depth (sum w_i d_i) in one pass, with an optional background colour
    added as (1 - opacity) * background.  radiance: float32[N, 4] with ray_hit = t_vals / step lengths float32[N], or
    float16[N, 4] with ray_hit = None (VR_COMPAT) / segment_step float32[P] (VR_NERF).  t_start, t_end: float32[P] segment
    entry / exit distances, needed for depth.  depth, opacity: float32[B] or None.  background: 3 floats or None."""
    layout = RADIANCE_HALF4 if radiance.dtype == torch.float16 else RADIANCE_FLOAT4
    bg = None
    if background is not None:
        bg = (C.c_float * 3)(*[float(v) for v in background])
    check(_lib.lib().rtxn_volrender_fwd_aux(_ptr(radiance, radiance.dtype if layout == RADIANCE_HALF4 else torch.float32, "radiance"),
                                            layout, _ptr(ray_hit, torch.float32, "ray_hit"),
                                            _ptr(num_hits, torch.int32, "num_hits"), _ptr(indices, torch.int32, "indices"),
                                            _ptr(t_start, torch.float32, "t_start"), _ptr(t_end, torch.float32, "t_end"),
                                            batch_size, num_samples_per_hit, mode, sample_type,
                                            C.cast(bg, C.c_void_p) if bg is not None else None,
                                            _ptr(pixels, torch.float32, "pixels"), _ptr(depth, torch.float32, "depth"),
                                            _ptr(opacity, torch.float32, "opacity"), _stream()),
          "rtxn_volrender_fwd_aux")
    return pixels, depth, opacity


def hashmlp_supported(net, grid):
    """True if the fused hash-encode + MLP inference kernel is built for this model / grid pair."""
    return bool(_lib.lib().rtxn_hashmlp_supported(net._h, grid._h, grid.n_dir_freqs))


def hashmlp_forward_segments(net, grid, table_fp16, start_points, end_points, seg_view, total_segments, max_segments, radiance_half4,
                             sample_type=SAMPLING_REGULAR, t_scale=1.0, segment_step=None):
    """launchSampler + HashGrid/Frequency encoding + network->forward + glue as one kernel over packed segments (the hash-grid
    counterpart of Network.forward_segments_compact): half[N, 4] radiance, optionally the per-segment world step."""
    check(_lib.lib().rtxn_hashmlp_forward_segments(
        net._h, grid._h, grid.n_dir_freqs, _ptr(table_fp16, torch.float16, "table"), _ptr(start_points, torch.float32, "start_points"),
        _ptr(end_points, torch.float32, "end_points"), _ptr(seg_view, torch.float32, "seg_view"),
        _ptr(total_segments, torch.int32, "total_segments"), int(max_segments), int(sample_type), float(t_scale),
        _ptr(radiance_half4, torch.float16, "radiance_half4"), _ptr(segment_step, torch.float32, "segment_step"), _stream()),
        "rtxn_hashmlp_forward_segments")
    return radiance_half4


# --------------------------------------------------------------------------- training path
def padded_samples(n):
    return int(_lib.lib().rtxn_padded_samples(n))


class HashGrid:
    """Multiresolution hash grid for positions (+ Frequency for directions)."""

    def __init__(self, n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.5,
                 n_dir_freqs=4):
        self.cfg = _lib.HashGridConfig(n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale)
        self.n_dir_freqs = n_dir_freqs
        h = C.c_void_p()
        check(_lib.lib().rtxn_hashgrid_create(C.byref(self.cfg), C.byref(h)), "rtxn_hashgrid_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.rtxn_hashgrid_destroy(h)

    def n_params(self):
        return int(_lib.lib().rtxn_hashgrid_n_params(self._h))

    def encoded_width(self):
        return int(_lib.lib().rtxn_hashgrid_encoded_width(self._h, self.n_dir_freqs))

    def level_offset(self, level):
        """Offset of `level` in table parameters (entries x features); level == n_levels: the total."""
        return int(_lib.lib().rtxn_hashgrid_level_offset(self._h, level))

    def hashed_offset(self):
        """Parameters before the first hashed level: the leading, densely stored levels (a few hundred KB)."""
        for l in range(self.cfg.n_levels):
            if _lib.lib().rtxn_hashgrid_level_is_hashed(self._h, l):
                return self.level_offset(l)
        return self.n_params()

    def encode(self, table_fp16, inputs, encT=None):
        n = inputs.numel() // 5
        if encT is None:
            encT = torch.empty((self.encoded_width(), padded_samples(n)), dtype=torch.float16, device=inputs.device)
        check(_lib.lib().rtxn_hashgrid_encode(self._h, self.n_dir_freqs, _ptr(table_fp16, torch.float16, "table"),
                                              _ptr(inputs, torch.float32, "inputs"), _ptr(encT, torch.float16, "encT"),
                                              n, _stream()), "rtxn_hashgrid_encode")
        return encT

    def encode_segments(self, table_fp16, start_points, end_points, seg_view, n_segments, sample_type, encT, t_vals=None, t_scale=1.0,
                        jitter=None):
        """launchSampler + encode in one pass over the packed segments (the float[S][5] samples are never written).
        jitter: sample_jitter(...) with SAMPLING_JITTER_WORLD -> the _jitter entry point (here and in every method that takes it)."""
        args = (self._h, self.n_dir_freqs, _ptr(table_fp16, torch.float16, "table"),
                _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points"),
                _ptr(seg_view, torch.float32, "seg_view"), n_segments, sample_type, t_scale,
                _ptr(encT, torch.float16, "encT"), _ptr(t_vals, torch.float32, "t_vals"))
        if jitter is not None:
            check(_lib.lib().rtxn_hashgrid_encode_segments_jitter(*args, _jit(jitter), _stream()), "rtxn_hashgrid_encode_segments_jitter")
        else:
            check(_lib.lib().rtxn_hashgrid_encode_segments(*args, _stream()), "rtxn_hashgrid_encode_segments")
        return encT

    def backward_segments(self, start_points, end_points, n_segments, sample_type, dencT, dtable, dtable_hashed_half=None, live_ws=None,
                          jitter=None):
        """live_ws (from live_segments): visit only the segments that carry a loss gradient."""
        head = (self._h, _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points"), n_segments,
                sample_type, _ptr(dencT, torch.float16, "dencT"))
        tail = (_ptr(dtable, torch.float32, "dtable"), _ptr(dtable_hashed_half, torch.float16, "dtable_hashed_half"))
        tail += (_jit(jitter), _stream()) if jitter is not None else (_stream(),)
        name = "rtxn_hashgrid_backward_segments" + ("_live" if live_ws is not None else "") + ("_jitter" if jitter is not None else "")
        if live_ws is not None:
            head += (_ptr(live_ws, None, "live_ws"),)
        check(getattr(_lib.lib(), name)(*head, *tail), name)
        return dtable

    def input_gradient_segments(self, table_fp16, start_points, end_points, n_segments, sample_type, dencT, dstart, dend, **kw):
        """hashgrid_input_gradient_segments(self, ...): dL/d(position) reduced to the segments' end points."""
        return hashgrid_input_gradient_segments(self, table_fp16, start_points, end_points, n_segments, sample_type, dencT, dstart, dend, **kw)

    def backward_mixed(self, inputs, dencT, dtable, dtable_hashed_half):
        """backward with the hashed levels' gradient accumulated in fp16 (packed atomics; n_features == 2)."""
        n = inputs.numel() // 5
        check(_lib.lib().rtxn_hashgrid_backward_mixed(self._h, _ptr(inputs, torch.float32, "inputs"), _ptr(dencT, torch.float16, "dencT"),
                                                      n, _ptr(dtable, torch.float32, "dtable"),
                                                      _ptr(dtable_hashed_half, torch.float16, "dtable_hashed_half"), _stream()),
              "rtxn_hashgrid_backward_mixed")
        return dtable

    def backward(self, inputs, dencT, dtable):
        n = inputs.numel() // 5
        check(_lib.lib().rtxn_hashgrid_backward(self._h, _ptr(inputs, torch.float32, "inputs"),
                                                _ptr(dencT, torch.float16, "dencT"), n,
                                                _ptr(dtable, torch.float32, "dtable"), _stream()),
              "rtxn_hashgrid_backward")
        return dtable


def _net_encode_frequency(self, inputs, encT=None):
    n = inputs.numel() // 5
    if encT is None:
        encT = torch.empty((self.encoded_width(), padded_samples(n)), dtype=torch.float16, device=inputs.device)
    check(_lib.lib().rtxn_encode_frequency(self._h, _ptr(inputs, torch.float32, "inputs"), _ptr(encT, torch.float16),
                                           n, _stream()), "rtxn_encode_frequency")
    return encT


def _net_encode_frequency_segments(self, start_points, end_points, seg_view, n_segments, sample_type, encT, t_vals=None, t_scale=1.0,
                                   jitter=None):
    """launchSampler + Composite-Frequency encoding in one pass over the packed segments."""
    args = (self._h, _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points"),
            _ptr(seg_view, torch.float32, "seg_view"), n_segments, sample_type, t_scale, _ptr(encT, torch.float16, "encT"),
            _ptr(t_vals, torch.float32, "t_vals"))
    if jitter is not None:
        check(_lib.lib().rtxn_encode_frequency_segments_jitter(*args, _jit(jitter), _stream()), "rtxn_encode_frequency_segments_jitter")
    else:
        check(_lib.lib().rtxn_encode_frequency_segments(*args, _stream()), "rtxn_encode_frequency_segments")
    return encT


def _net_train_workspace(self, n, device="cuda"):
    nbytes = _lib.lib().rtxn_mlp_train_workspace_bytes(self._h, n)
    return torch.empty(nbytes // 2, dtype=torch.float16, device=device)


def _net_train_forward(self, encT, n, workspace, output=None, radiance=None):
    """network->forward(stream, input, &output, use_inference_params=false, prepare_input_gradients) (main.cu:721)."""
    if output is None:
        output = torch.empty((n, 16), dtype=torch.float16, device=encT.device)
    check(_lib.lib().rtxn_mlp_train_forward(self._h, _ptr(encT, torch.float16, "encT"), n, _ptr(workspace, torch.float16),
                                            _ptr(output, torch.float16), _ptr(radiance, torch.float32, "radiance"),
                                            _stream()), "rtxn_mlp_train_forward")
    return output


def _net_train_backward(self, encT, output, dout, n, workspace, dparams, dencT=None):
    """network->backward(stream, ctx, input, output, dL_doutput) (main.cu:781)."""
    check(_lib.lib().rtxn_mlp_train_backward(self._h, _ptr(encT, torch.float16, "encT"), _ptr(output, torch.float16, "output"),
                                             _ptr(dout, torch.float16, "dout"), n, _ptr(workspace, torch.float16),
                                             _ptr(dparams, torch.float32, "dparams"), _ptr(dencT, torch.float16, "dencT"),
                                             _stream()), "rtxn_mlp_train_backward")
    return dparams


def _net_recompute_supported(self):
    """True for models whose backward can run as the fused recompute kernel (64 wide, <= 4 layers, encoded width <= 64)."""
    return bool(_lib.lib().rtxn_mlp_train_recompute_supported(self._h))


def _net_train_forward_outputs(self, encT, n, output=None, radiance=None):
    """network->forward without saved activations (the forward half of the recompute path)."""
    if output is None:
        output = torch.empty((n, 16), dtype=torch.float16, device=encT.device)
    check(_lib.lib().rtxn_mlp_train_forward_outputs(self._h, _ptr(encT, torch.float16, "encT"), n, _ptr(output, torch.float16),
                                                    _ptr(radiance, torch.float32, "radiance"), _stream()),
          "rtxn_mlp_train_forward_outputs")
    return output


def _net_train_backward_recompute(self, encT, output, dout, n, dparams, dencT=None):
    """network->backward as one kernel: activations rebuilt from encT, every weight gradient accumulated on the chip."""
    check(_lib.lib().rtxn_mlp_train_backward_recompute(self._h, _ptr(encT, torch.float16, "encT"), _ptr(output, torch.float16, "output"),
                                                       _ptr(dout, torch.float16, "dout"), n, _ptr(dparams, torch.float32, "dparams"),
                                                       _ptr(dencT, torch.float16, "dencT"), _stream()),
          "rtxn_mlp_train_backward_recompute")
    return dparams


Network.recompute_supported = _net_recompute_supported
Network.train_forward_outputs = _net_train_forward_outputs
Network.train_backward_recompute = _net_train_backward_recompute
Network.encode_frequency = _net_encode_frequency
Network.encode_frequency_segments = _net_encode_frequency_segments
def _net_train_backward_recompute_live(self, encT, output, dout, n, live_ws, dparams, dencT=None):
    check(_lib.lib().rtxn_mlp_train_backward_recompute_live(self._h, _ptr(encT, torch.float16, "encT"), _ptr(output, torch.float16, "output"),
                                                           _ptr(dout, torch.float16, "dout"), n, _ptr(live_ws, None, "live_ws"),
                                                           _ptr(dparams, torch.float32, "dparams"), _ptr(dencT, torch.float16, "dencT"),
                                                           _stream()), "rtxn_mlp_train_backward_recompute_live")


def _net_train_backward_live(self, encT, output, dout, n, workspace, live_ws, dparams, dencT=None):
    check(_lib.lib().rtxn_mlp_train_backward_live(self._h, _ptr(encT, torch.float16, "encT"), _ptr(output, torch.float16, "output"),
                                                 _ptr(dout, torch.float16, "dout"), n, _ptr(workspace, torch.float16, "workspace"),
                                                 _ptr(live_ws, None, "live_ws"), _ptr(dparams, torch.float32, "dparams"),
                                                 _ptr(dencT, torch.float16, "dencT"), _stream()), "rtxn_mlp_train_backward_live")


def _net_train_forward_live(self, encT, n, workspace, live_ws):
    """network->forward's SAVED ACTIVATIONS for the live segments only (the outputs come from train_forward_outputs)."""
    check(_lib.lib().rtxn_mlp_train_forward_live(self._h, _ptr(encT, torch.float16, "encT"), n, _ptr(workspace, torch.float16, "workspace"),
                                                 _ptr(live_ws, None, "live_ws"), _stream()), "rtxn_mlp_train_forward_live")


def _net_lean_supported(self):
    """True for models with the lean training path (the reference's 8 x 128 model): no saved activations, the weight gradient
    recomputes them (rtxn_mlp_train_lean_supported)."""
    return bool(_lib.lib().rtxn_mlp_train_lean_supported(self._h))


def _net_train_lean_workspace(self, n, device="cuda"):
    nbytes = _lib.lib().rtxn_mlp_train_lean_workspace_bytes(self._h, n)
    if nbytes == 0:
        raise _lib.RtxnError("train_lean_workspace: this model has no lean path")
    return torch.empty(nbytes // 2, dtype=torch.float16, device=device)


def _net_train_forward_lean(self, encT, n, workspace, output=None, radiance=None):
    """network->forward keeping outputs + sign masks only (rtxn_mlp_train_forward_lean)."""
    if output is None:
        output = torch.empty((n, 16), dtype=torch.float16, device=encT.device)
    check(_lib.lib().rtxn_mlp_train_forward_lean(self._h, _ptr(encT, torch.float16, "encT"), n, _ptr(workspace, torch.float16, "workspace"),
                                                 _ptr(output, torch.float16), _ptr(radiance, torch.float32, "radiance"), _stream()),
          "rtxn_mlp_train_forward_lean")
    return output


def _net_lean_fused_supported(self):
    """True where the lean forward can encode for itself (the reference's Composite-Frequency(3 x 10, 2 x 12) model)."""
    return bool(_lib.lib().rtxn_mlp_train_forward_lean_fused_supported(self._h))


def _net_train_forward_lean_segments(self, start_points, end_points, seg_view, n_segments, sample_type, workspace, output, radiance=None,
                                     t_vals=None, t_scale=1.0, jitter=None):
    """The lean forward with sampler and encoder folded in (rtxn_mlp_train_forward_lean_segments): encT is not read; t_vals as the
    standalone encoder writes them."""
    args = (self._h, _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points"),
            _ptr(seg_view, torch.float32, "seg_view"), n_segments, sample_type, t_scale, _ptr(t_vals, torch.float32, "t_vals"),
            _ptr(workspace, torch.float16, "workspace"), _ptr(output, torch.float16), _ptr(radiance, torch.float32, "radiance"))
    if jitter is not None:
        check(_lib.lib().rtxn_mlp_train_forward_lean_segments_jitter(*args, _jit(jitter), _stream()),
              "rtxn_mlp_train_forward_lean_segments_jitter")
    else:
        check(_lib.lib().rtxn_mlp_train_forward_lean_segments(*args, _stream()), "rtxn_mlp_train_forward_lean_segments")
    return output


def _net_train_backward_lean_segments(self, start_points, end_points, seg_view, n_segments, sample_type, output, dout, workspace, dparams,
                                      live_ws=None, jitter=None):
    """The lean backward whose weight gradient recomputes the encoding as well (rtxn_mlp_train_backward_lean_segments): no encT."""
    args = (self._h, _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points"),
            _ptr(seg_view, torch.float32, "seg_view"), n_segments, sample_type, _ptr(output, torch.float16), _ptr(dout, torch.float16),
            _ptr(workspace, torch.float16, "workspace"), _ptr(live_ws, None, "live_ws"), _ptr(dparams, torch.float32))
    if jitter is not None:
        check(_lib.lib().rtxn_mlp_train_backward_lean_segments_jitter(*args, _jit(jitter), _stream()),
              "rtxn_mlp_train_backward_lean_segments_jitter")
    else:
        check(_lib.lib().rtxn_mlp_train_backward_lean_segments(*args, _stream()), "rtxn_mlp_train_backward_lean_segments")
    return dparams


def _net_train_backward_lean(self, encT, output, dout, n, workspace, dparams, live_ws=None):
    """network->backward on the lean workspace: dgrad chain + weight gradient with recomputed activations."""
    check(_lib.lib().rtxn_mlp_train_backward_lean(self._h, _ptr(encT, torch.float16, "encT"), _ptr(output, torch.float16, "output"),
                                                  _ptr(dout, torch.float16, "dout"), n, _ptr(workspace, torch.float16, "workspace"),
                                                  _ptr(live_ws, None, "live_ws"), _ptr(dparams, torch.float32, "dparams"), _stream()),
          "rtxn_mlp_train_backward_lean")
    return dparams


Network.lean_supported = _net_lean_supported
Network.train_lean_workspace = _net_train_lean_workspace
Network.train_forward_lean = _net_train_forward_lean
Network.lean_fused_supported = _net_lean_fused_supported
Network.train_forward_lean_segments = _net_train_forward_lean_segments
Network.train_backward_lean_segments = _net_train_backward_lean_segments
Network.train_backward_lean = _net_train_backward_lean
Network.train_forward_live = _net_train_forward_live
Network.train_backward_recompute_live = _net_train_backward_recompute_live
Network.train_backward_live = _net_train_backward_live
Network.train_workspace = _net_train_workspace
Network.train_forward = _net_train_forward
Network.train_backward = _net_train_backward


def l2_loss(pred, target, loss_scale=1.0, values=None, grads=None, loss_sum=None):
    """loss->evaluate(loss_scale, prediction, target, values, gradients) (main.cu:759)."""
    n = pred.numel()
    check(_lib.lib().rtxn_l2_loss(_ptr(pred, torch.float32, "pred"), _ptr(target, torch.float32, "target"), n, loss_scale,
                                  _ptr(values, torch.float32, "values"), _ptr(grads, torch.float16, "grads"),
                                  _ptr(loss_sum, torch.float32, "loss_sum"), _stream()), "rtxn_l2_loss")


def loss(pred, target, spec, loss_scale=1.0, values=None, grads=None, loss_sum=None):
    """l2_loss for the four kinds (spec: train_loss(...) without an alpha term): rtxn_loss, elementwise over pred.numel() values."""
    check(_lib.lib().rtxn_loss(_ptr(pred, torch.float32, "pred"), _ptr(target, torch.float32, "target"), pred.numel(), _byref(spec),
                               loss_scale, _ptr(values, torch.float32, "values"), _ptr(grads, torch.float16, "grads"),
                               _ptr(loss_sum, torch.float32, "loss_sum"), _stream()), "rtxn_loss")


def adam_step(master, params_fp16, grads, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, loss_scale=1.0):
    """optimizer->step(stream, loss_scale, params_fp32, params, gradients) (main.cu:787)."""
    check(_lib.lib().rtxn_adam_step(master.numel(), _ptr(master, torch.float32, "master"),
                                    _ptr(params_fp16, torch.float16, "params"), _ptr(grads, torch.float32, "grads"),
                                    _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"), step, lr, beta1, beta2, eps,
                                    loss_scale, _stream()), "rtxn_adam_step")


def adam_step_half_grads(master, params_fp16, grads_fp16, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, loss_scale=1.0):
    """adam_step with an fp16 gradient."""
    check(_lib.lib().rtxn_adam_step_half_grads(master.numel(), _ptr(master, torch.float32, "master"),
                                               _ptr(params_fp16, torch.float16, "params"), _ptr(grads_fp16, torch.float16, "grads"),
                                               _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"), step, lr, beta1, beta2, eps,
                                               loss_scale, _stream()), "rtxn_adam_step_half_grads")


def adam_effective_lr(lr, beta1, beta2, step):
    """The bias-corrected rate rtxn_adam_step uses at `step` (computed by the library, so the captured form is bit-identical)."""
    return float(_lib.lib().rtxn_adam_effective_lr(lr, beta1, beta2, int(step)))


ADAM_GRADS_FP16, ADAM_ZERO_GRADS = 1, 2


def adam_step_captured(master, params_fp16, grads, m, v, effective_lr, beta1=0.9, beta2=0.999, eps=1e-8, loss_scale=1.0, zero_grads=False):
    """adam_step / adam_step_half_grads (by the dtype of `grads`) with the bias-corrected rate read from the device float
    `effective_lr`: the form a hipGraph can replay.  zero_grads: clear the gradient as it is consumed."""
    half = grads.dtype == torch.float16
    flags = (ADAM_GRADS_FP16 if half else 0) | (ADAM_ZERO_GRADS if zero_grads else 0)
    check(_lib.lib().rtxn_adam_step_captured(master.numel(), _ptr(master, torch.float32, "master"),
                                             _ptr(params_fp16, torch.float16, "params"),
                                             _ptr(grads, torch.float16 if half else torch.float32, "grads"), flags,
                                             _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"),
                                             _ptr(effective_lr, torch.float32, "effective_lr"), beta1, beta2, eps, loss_scale,
                                             _stream()), "rtxn_adam_step_captured")


def adam_step_sparse(master, params_fp16, grads, m, v, param_steps, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, loss_scale=1.0,
                     zero_grads=False):
    """rtxn_adam_step_sparse: tiny-cuda-nn's Adam for the hash table -- entries with a zero gradient are skipped, bias correction
    by the entry's own update count (param_steps, int32/uint32[n]).  grads: fp32 or fp16."""
    half = grads.dtype == torch.float16
    flags = (ADAM_GRADS_FP16 if half else 0) | (ADAM_ZERO_GRADS if zero_grads else 0)
    check(_lib.lib().rtxn_adam_step_sparse(master.numel(), _ptr(master, torch.float32, "master"),
                                           _ptr(params_fp16, torch.float16, "params"),
                                           _ptr(grads, torch.float16 if half else torch.float32, "grads"), flags,
                                           _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"),
                                           _ptr(param_steps, torch.int32, "param_steps"), lr, beta1, beta2, eps, loss_scale,
                                           _stream()), "rtxn_adam_step_sparse")


# --------------------------------------------------------------------------- optimizer options
LR_CONSTANT, LR_EXPONENTIAL, LR_COSINE = 0, 1, 2
_LR_KINDS = {"constant": LR_CONSTANT, "exponential": LR_EXPONENTIAL, "cosine": LR_COSINE}
# "nerf": x0.1 per 250k steps (the reference's own comment, main.cu:39, is this decay from 5e-4 to 5e-5);
# "instant_ngp": x0.33 every 10k steps after the first 20k
LR_PRESETS = {"nerf": dict(kind="exponential", decay_steps=250000, ratio=0.1),
              "instant_ngp": dict(kind="exponential", decay_start=20000, decay_steps=10000, ratio=0.33, staircase=True)}
ADAM_NO_WEIGHT_DECAY = 4


def lr_schedule(kind="constant", warmup_steps=0, decay_start=0, decay_steps=0, ratio=1.0, staircase=False):
    """struct rtxn_lr_schedule (include/rtxn.h): factor(t) = warm(t) dec(t) on the learning rates of update t (1-based), evaluated
    on the device from the step counter.  kind: "constant", "exponential" (ratio^x, x = max(0, t - decay_start) / decay_steps;
    staircase: floor(x)) or "cosine" (from 1 to ratio over decay_steps), or one of LR_PRESETS ("nerf", "instant_ngp") with the
    other arguments overriding it; warmup_steps: linear warm-up.  Accepts a dict of these arguments, or a struct, as well."""
    if isinstance(kind, _lib.LrSchedule):
        return kind
    if isinstance(kind, dict):
        return lr_schedule(**kind)
    kw = dict(warmup_steps=warmup_steps, decay_start=decay_start, decay_steps=decay_steps, ratio=ratio, staircase=staircase)
    if kind in LR_PRESETS:
        preset = dict(LR_PRESETS[kind])
        defaults = dict(warmup_steps=0, decay_start=0, decay_steps=0, ratio=1.0, staircase=False)
        kw = {**defaults, **preset, **{k: v for k, v in kw.items() if v != defaults[k]}}
        kind = kw.pop("kind")
    if isinstance(kind, str):
        if kind not in _LR_KINDS:
            raise ValueError(f"lr_schedule: kind {kind!r}: one of {sorted(_LR_KINDS) + sorted(LR_PRESETS)}")
        kind = _LR_KINDS[kind]
    s = _lib.LrSchedule()
    s.kind, s.warmup_steps, s.decay_start, s.decay_steps = int(kind), int(kw["warmup_steps"]), int(kw["decay_start"]), int(kw["decay_steps"])
    s.ratio, s.staircase = float(kw["ratio"]), int(bool(kw["staircase"]))
    return s


def lr_schedule_factor(schedule, step):
    """rtxn_lr_schedule_factor: factor(step) on the host, the definition the device restates (for logging)."""
    sch = lr_schedule(schedule)
    f = _lib.lib().rtxn_lr_schedule_factor(C.byref(sch), int(step))
    if f < 0.0:               # a schedule that breaks the rules, or step < 1: the message is the library's
        check(1, "rtxn_lr_schedule_factor")
    return float(f)


def optimizer_options(schedule=None, weight_decay=0.0, skip_nonfinite=False, lr_factor=None, guard=None):
    """struct rtxn_optimizer_options (include/rtxn.h).  lr_factor: device float32[1] scratch; guard: device int32[4], zeroed:
    [0] the non-finite flag, [1] skipped steps, [2] this step's skip word.  The tensors stay referenced by the struct."""
    o = _lib.OptimizerOptions()
    o.schedule = lr_schedule(schedule) if schedule is not None else lr_schedule()
    o.weight_decay, o.skip_nonfinite = float(weight_decay), int(bool(skip_nonfinite))
    o.lr_factor, o.guard = _ptr(lr_factor, torch.float32, "lr_factor"), _ptr(guard, torch.int32, "guard")
    if guard is not None and guard.numel() < 4:
        raise _lib.RtxnError(f"optimizer_options: guard holds {guard.numel()} words, 4 are needed")
    o._tensors = (lr_factor, guard)
    return o


def optimizer_options_check(opt):
    """rtxn_optimizer_options_check: the struct's rules without its two pointers; needs no device."""
    check(_lib.lib().rtxn_optimizer_options_check(_byref(opt)), "rtxn_optimizer_options_check")


def optimizer_rate(opt, step, effective_lr, lr=1e-3, table_lr=0.0, table_effective_lr=None, advance=True, beta1=0.9, beta2=0.999):
    """rtxn_optimizer_rate: the one-thread kernel that (advances and) reads the device int32 `step`, writes factor(t) to the
    options' lr_factor, the bias-corrected rate(s) to effective_lr (and table_effective_lr) and moves the guard words."""
    check(_lib.lib().rtxn_optimizer_rate(C.byref(opt), _ptr(step, torch.int32, "step"), int(bool(advance)), lr, table_lr, beta1, beta2,
                                         _ptr(effective_lr, torch.float32, "effective_lr"),
                                         _ptr(table_effective_lr, torch.float32, "table_effective_lr"), _stream()), "rtxn_optimizer_rate")


def _grad_buffers(buffers):
    """(struct rtxn_grad_buffer array, its length) over the fp32 / fp16 tensors in `buffers`; None and empty ones are skipped"""
    bufs = [b for b in buffers if b is not None and b.numel()]
    arr = (_lib.GradBuffer * max(1, len(bufs)))()
    for k, b in enumerate(bufs):
        half = b.dtype == torch.float16
        arr[k].data, arr[k].count, arr[k].is_fp16 = _ptr(b, torch.float16 if half else torch.float32, "buffers[%d]" % k), b.numel(), int(half)
    return arr, len(bufs)


def check_gradients(buffers, flag):
    """rtxn_check_gradients: OR the device int32 `flag` (an options' guard) if any element of the fp32 / fp16 tensors in `buffers`
    (at most 4; None and empty ones are skipped) is Inf or NaN."""
    arr, n = _grad_buffers(buffers)
    check(_lib.lib().rtxn_check_gradients(arr, n, _ptr(flag, torch.int32, "flag"), _stream()), "rtxn_check_gradients")


def adam_step_opt(master, params_fp16, grads, m, v, effective_lr, opt, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, loss_scale=1.0,
                  zero_grads=False, weight_decay=True):
    """rtxn_adam_step_opt: adam_step_captured under optimizer_options(...) -- the decay term uses lr * factor, the skip word is
    honoured.  weight_decay=False: this call does not decay (the hash table)."""
    half = grads.dtype == torch.float16
    flags = (ADAM_GRADS_FP16 if half else 0) | (ADAM_ZERO_GRADS if zero_grads else 0) | (0 if weight_decay else ADAM_NO_WEIGHT_DECAY)
    check(_lib.lib().rtxn_adam_step_opt(master.numel(), _ptr(master, torch.float32, "master"), _ptr(params_fp16, torch.float16, "params"),
                                        _ptr(grads, torch.float16 if half else torch.float32, "grads"), flags,
                                        _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"),
                                        _ptr(effective_lr, torch.float32, "effective_lr"), lr, beta1, beta2, eps, loss_scale,
                                        _byref(opt), _stream()), "rtxn_adam_step_opt")


def adam_step_sparse_opt(master, params_fp16, grads, m, v, param_steps, opt, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, loss_scale=1.0,
                         zero_grads=False, weight_decay=True):
    """rtxn_adam_step_sparse_opt: adam_step_sparse under optimizer_options(...): lr * factor, the skip word, and the decay term
    on the entries it updates (weight_decay=False: none)."""
    half = grads.dtype == torch.float16
    flags = (ADAM_GRADS_FP16 if half else 0) | (ADAM_ZERO_GRADS if zero_grads else 0) | (0 if weight_decay else ADAM_NO_WEIGHT_DECAY)
    check(_lib.lib().rtxn_adam_step_sparse_opt(master.numel(), _ptr(master, torch.float32, "master"),
                                               _ptr(params_fp16, torch.float16, "params"),
                                               _ptr(grads, torch.float16 if half else torch.float32, "grads"), flags,
                                               _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"),
                                               _ptr(param_steps, torch.int32, "param_steps"), lr, beta1, beta2, eps, loss_scale,
                                               _byref(opt), _stream()), "rtxn_adam_step_sparse_opt")


# --------------------------------------------------------------------------- dynamic loss scale, gradient clipping
def loss_scaler(init_scale=128.0, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=65536.0, max_grad_norm=0.0,
                state=None, partials=None):
    """struct rtxn_loss_scaler (include/rtxn.h): the loss scale kept in device memory -- halved (backoff) when a step's gradients
    are not finite, doubled (growth) after growth_interval clean steps, inside [min_scale, max_scale] -- and gradient-norm clipping
    at max_grad_norm (0: none; torch.nn.utils.clip_grad_norm_'s rule).  The five scales and factors are exact powers of two.
    state: device int32[8] (loss_scaler_state_tensor); partials: device float64 workspace (loss_scaler_workspace); both stay
    referenced by the struct.  Accepts a dict of these arguments, or a struct, as well.  The rules are the library's
    (rtxn_loss_scaler_check), applied here, before anything touches a device."""
    if isinstance(init_scale, _lib.LossScaler):
        return init_scale
    if isinstance(init_scale, dict):
        return loss_scaler(**init_scale)
    s = _lib.LossScaler()
    s.init_scale, s.growth, s.backoff, s.growth_interval = float(init_scale), float(growth), float(backoff), int(growth_interval)
    s.min_scale, s.max_scale, s.max_grad_norm = float(min_scale), float(max_scale), float(max_grad_norm)
    if int(growth_interval) != growth_interval:
        raise _lib.RtxnError(f"loss_scaler: growth_interval = {growth_interval!r} is not an integer")
    check(_lib.lib().rtxn_loss_scaler_check(C.byref(s)), "rtxn_loss_scaler_check")
    if state is not None and state.numel() < 8:
        raise _lib.RtxnError(f"loss_scaler: state holds {state.numel()} words, 8 are needed")
    if partials is not None and partials.numel() * 8 < _lib.lib().rtxn_loss_scaler_workspace_bytes():
        raise _lib.RtxnError(f"loss_scaler: partials holds {partials.numel()} doubles, "
                             f"{_lib.lib().rtxn_loss_scaler_workspace_bytes() // 8} are needed")
    s.state, s.partials = _ptr(state, torch.int32, "state"), _ptr(partials, torch.float64, "partials")
    s._tensors = (state, partials)
    return s


def loss_scaler_initial_state(scaler):
    """rtxn_loss_scaler_init_state: the eight words a run starts from, as a numpy int32[8] (view float32 for words 0, 1 and 6)."""
    st = _lib.LossScalerState()
    check(_lib.lib().rtxn_loss_scaler_init_state(C.byref(scaler), C.byref(st)), "rtxn_loss_scaler_init_state")
    return np.frombuffer(bytes(st), dtype=np.int32).copy()


def loss_scaler_state_tensor(scaler, device="cuda"):
    """device int32[8] holding the initial state of `scaler`"""
    return torch.from_numpy(loss_scaler_initial_state(scaler)).to(device)


def loss_scaler_workspace(device="cuda"):
    """device float64 workspace of the statistics kernel's per-block sums (rtxn_loss_scaler_workspace_bytes)"""
    return torch.zeros(_lib.lib().rtxn_loss_scaler_workspace_bytes() // 8, dtype=torch.float64, device=device)


def loss_scaler_advance(scaler, state, flag, sumsq, divisor=1.0):
    """rtxn_loss_scaler_advance: the device's state machine on the host.  state: a _lib.LossScalerState; returns the next one."""
    out = _lib.LossScalerState()
    check(_lib.lib().rtxn_loss_scaler_advance(C.byref(scaler), C.byref(state), int(bool(flag)), float(sumsq), float(divisor), C.byref(out)),
          "rtxn_loss_scaler_advance")
    return out


def gradient_statistics(buffers, flag, scaler):
    """rtxn_gradient_statistics: check_gradients' pass plus one double sum of squares per block, left in the scaler's partials
    at [buffer][block] (GRAD_STATS_MAX_BLOCKS per buffer)."""
    arr, n = _grad_buffers(buffers)
    check(_lib.lib().rtxn_gradient_statistics(arr, n, _ptr(flag, torch.int32, "flag"), C.byref(scaler), _stream()), "rtxn_gradient_statistics")


GRAD_STATS_MAX_BLOCKS = 2048


def loss_scaler_step(opt, scaler, buffers, step, effective_lr, lr=1e-3, table_lr=0.0, table_effective_lr=None, advance=True, beta1=0.9,
                     beta2=0.999, divisor=1.0):
    """rtxn_loss_scaler_step: optimizer_rate's one-block sibling -- reduces the partials gradient_statistics left for these same
    `buffers`, does what optimizer_rate does, then moves the scaler's device state (divisor: ranks summed into the gradients)."""
    arr, n = _grad_buffers(buffers)
    check(_lib.lib().rtxn_loss_scaler_step(C.byref(opt), C.byref(scaler), arr, n, _ptr(step, torch.int32, "step"), int(bool(advance)), lr,
                                           table_lr, beta1, beta2, _ptr(effective_lr, torch.float32, "effective_lr"),
                                           _ptr(table_effective_lr, torch.float32, "table_effective_lr"), float(divisor), _stream()),
          "rtxn_loss_scaler_step")


def adam_step_scaled(master, params_fp16, grads, m, v, effective_lr, opt, scaler, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                     zero_grads=False, weight_decay=True):
    """rtxn_adam_step_scaled: adam_step_opt with the factor on the raw gradient read from the scaler's device multiplier."""
    half = grads.dtype == torch.float16
    flags = (ADAM_GRADS_FP16 if half else 0) | (ADAM_ZERO_GRADS if zero_grads else 0) | (0 if weight_decay else ADAM_NO_WEIGHT_DECAY)
    check(_lib.lib().rtxn_adam_step_scaled(master.numel(), _ptr(master, torch.float32, "master"), _ptr(params_fp16, torch.float16, "params"),
                                           _ptr(grads, torch.float16 if half else torch.float32, "grads"), flags,
                                           _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"),
                                           _ptr(effective_lr, torch.float32, "effective_lr"), lr, beta1, beta2, eps,
                                           _byref(opt), _byref(scaler), _stream()), "rtxn_adam_step_scaled")


def adam_step_sparse_scaled(master, params_fp16, grads, m, v, param_steps, opt, scaler, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                            zero_grads=False, weight_decay=True):
    """rtxn_adam_step_sparse_scaled: adam_step_sparse_opt with the factor read from the scaler's device multiplier."""
    half = grads.dtype == torch.float16
    flags = (ADAM_GRADS_FP16 if half else 0) | (ADAM_ZERO_GRADS if zero_grads else 0) | (0 if weight_decay else ADAM_NO_WEIGHT_DECAY)
    check(_lib.lib().rtxn_adam_step_sparse_scaled(master.numel(), _ptr(master, torch.float32, "master"),
                                                  _ptr(params_fp16, torch.float16, "params"),
                                                  _ptr(grads, torch.float16 if half else torch.float32, "grads"), flags,
                                                  _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"),
                                                  _ptr(param_steps, torch.int32, "param_steps"), lr, beta1, beta2, eps,
                                                  _byref(opt), _byref(scaler), _stream()), "rtxn_adam_step_sparse_scaled")


# --------------------------------------------------------------------------- exponential moving average of the weights
def weight_ema(decay, state=None, mlp_ema=None, table_ema=None, table_stamps=None):
    """struct rtxn_weight_ema (include/rtxn.h): the debiased EMA of the weights, s = d s + (1 - d) w after every APPLIED update,
    read out as s / (1 - d^u).  state: device int32[4], zeroed (updates, correction as float32 bits, two reserved words); mlp_ema,
    table_ema: device float32 accumulators, zeroed; table_stamps: device int32 per table parameter, zeroed -- the update at which
    an entry's s was last current, for the sparse table rule, which keeps the average lazily (None: dense).  The tensors stay
    referenced by the struct.  The rule is the library's (rtxn_weight_ema_check), applied here, before anything touches a device."""
    if isinstance(decay, _lib.WeightEma):
        return decay
    e = _lib.WeightEma()
    e.decay = float(decay)
    check(_lib.lib().rtxn_weight_ema_check(C.byref(e)), "rtxn_weight_ema_check")
    if state is not None and state.numel() < 4:
        raise _lib.RtxnError(f"weight_ema: state holds {state.numel()} words, 4 are needed")
    if table_stamps is not None and (table_ema is None or table_stamps.numel() != table_ema.numel()):
        raise _lib.RtxnError("weight_ema: table_stamps without a table_ema of the same size")
    e.state, e.mlp_ema = _ptr(state, torch.int32, "state"), _ptr(mlp_ema, torch.float32, "mlp_ema")
    e.table_ema, e.table_stamps = _ptr(table_ema, torch.float32, "table_ema"), _ptr(table_stamps, torch.int32, "table_stamps")
    e._tensors = (state, mlp_ema, table_ema, table_stamps)
    return e


def ema_catch_up(s, w, gap, decay):
    """rtxn_ema_catch_up: the device's lazy catch-up on the host -- s after `gap` updates during which the weight stayed w."""
    weight_ema(decay)                         # the rule; a NaN below is then the arithmetic's own (inf - inf)
    return float(_lib.lib().rtxn_ema_catch_up(float(s), float(w), int(gap), float(decay)))


def ema_correction(decay, updates):
    """rtxn_ema_correction: (float)(1 / (1 - d^updates)), the read-out's debias factor; updates = 0 gives 1."""
    r = _lib.lib().rtxn_ema_correction(float(decay), int(updates))
    if r < 0.0:
        check(1, "rtxn_ema_correction")
    return float(r)


def optimizer_rate_ema(opt, ema, step, effective_lr, lr=1e-3, table_lr=0.0, table_effective_lr=None, advance=True, beta1=0.9, beta2=0.999):
    """rtxn_optimizer_rate_ema: optimizer_rate that also advances the EMA's update count (unless the step is skipped) and writes
    its debias factor.  `opt` may have nothing switched on but needs lr_factor."""
    check(_lib.lib().rtxn_optimizer_rate_ema(C.byref(opt), _byref(ema), _ptr(step, torch.int32, "step"), int(bool(advance)), lr, table_lr,
                                             beta1, beta2, _ptr(effective_lr, torch.float32, "effective_lr"),
                                             _ptr(table_effective_lr, torch.float32, "table_effective_lr"), _stream()), "rtxn_optimizer_rate_ema")


def loss_scaler_step_ema(opt, scaler, ema, buffers, step, effective_lr, lr=1e-3, table_lr=0.0, table_effective_lr=None, advance=True,
                         beta1=0.9, beta2=0.999, divisor=1.0):
    """rtxn_loss_scaler_step_ema: loss_scaler_step that also advances the EMA's state."""
    arr, n = _grad_buffers(buffers)
    check(_lib.lib().rtxn_loss_scaler_step_ema(_byref(opt), _byref(scaler), _byref(ema), arr, n, _ptr(step, torch.int32, "step"),
                                               int(bool(advance)), lr, table_lr, beta1, beta2, _ptr(effective_lr, torch.float32, "effective_lr"),
                                               _ptr(table_effective_lr, torch.float32, "table_effective_lr"), float(divisor), _stream()),
          "rtxn_loss_scaler_step_ema")


def _ema_acc(who, acc, master, dtype=torch.float32, name="ema_acc", ema=True):
    if ema is None and acc is None:           # no EMA: the call without _ema
        return None
    if acc is None or acc.numel() != master.numel():
        raise _lib.RtxnError(f"{who}: {name} must hold one element per parameter ({master.numel()})")
    return _ptr(acc, dtype, name)


def adam_step_ema(master, params_fp16, grads, m, v, effective_lr, opt, ema, ema_acc, scaler=None, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                  loss_scale=1.0, zero_grads=False, weight_decay=True):
    """rtxn_adam_step_ema: adam_step_scaled (scaler=None: adam_step_opt) that also keeps s = d s + (1 - d) w of the parameters it
    steps in ema_acc (the dense form)."""
    half = grads.dtype == torch.float16
    flags = (ADAM_GRADS_FP16 if half else 0) | (ADAM_ZERO_GRADS if zero_grads else 0) | (0 if weight_decay else ADAM_NO_WEIGHT_DECAY)
    check(_lib.lib().rtxn_adam_step_ema(master.numel(), _ptr(master, torch.float32, "master"), _ptr(params_fp16, torch.float16, "params"),
                                        _ptr(grads, torch.float16 if half else torch.float32, "grads"), flags,
                                        _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"),
                                        _ptr(effective_lr, torch.float32, "effective_lr"), lr, beta1, beta2, eps, loss_scale,
                                        _byref(opt), _byref(scaler), _byref(ema), _ema_acc("adam_step_ema", ema_acc, master, ema=ema), _stream()),
          "rtxn_adam_step_ema")


def adam_step_sparse_ema(master, params_fp16, grads, m, v, param_steps, opt, ema, ema_acc, ema_stamps, scaler=None, lr=1e-3, beta1=0.9,
                         beta2=0.999, eps=1e-8, loss_scale=1.0, zero_grads=False, weight_decay=True):
    """rtxn_adam_step_sparse_ema: adam_step_sparse_scaled (scaler=None: adam_step_sparse_opt) that keeps the average lazily: the
    entries it updates are caught up over the updates they sat out (ema_stamps), then averaged."""
    half = grads.dtype == torch.float16
    flags = (ADAM_GRADS_FP16 if half else 0) | (ADAM_ZERO_GRADS if zero_grads else 0) | (0 if weight_decay else ADAM_NO_WEIGHT_DECAY)
    who = "adam_step_sparse_ema"
    check(_lib.lib().rtxn_adam_step_sparse_ema(master.numel(), _ptr(master, torch.float32, "master"),
                                               _ptr(params_fp16, torch.float16, "params"),
                                               _ptr(grads, torch.float16 if half else torch.float32, "grads"), flags,
                                               _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"),
                                               _ptr(param_steps, torch.int32, "param_steps"), lr, beta1, beta2, eps, loss_scale,
                                               _byref(opt), _byref(scaler), _byref(ema), _ema_acc(who, ema_acc, master, ema=ema),
                                               _ema_acc(who, ema_stamps, master, torch.int32, "ema_stamps", ema=ema), _stream()),
          "rtxn_adam_step_sparse_ema")


def ema_weights(master, ema_acc, stamps, state, decay, out_f32=None, out_f16=None):
    """rtxn_ema_weights: the debiased average of `master`'s parameters from their accumulator (and stamps: the lazy form; None:
    dense) into out_f32 and / or out_f16.  Pure: the training state is only read."""
    who = "ema_weights"
    for nm, t in (("out_f32", out_f32), ("out_f16", out_f16)):
        if t is not None and t.numel() != master.numel():
            raise _lib.RtxnError(f"{who}: {nm} holds {t.numel()} elements, {master.numel()} parameters")
    if state is None or state.numel() < 4:
        raise _lib.RtxnError(f"{who}: state must hold 4 words")
    check(_lib.lib().rtxn_ema_weights(master.numel(), _ptr(master, torch.float32, "master"), _ema_acc(who, ema_acc, master),
                                      _ema_acc(who, stamps, master, torch.int32, "stamps") if stamps is not None else None,
                                      _ptr(state, torch.int32, "state"), float(decay), _ptr(out_f32, torch.float32, "out_f32"),
                                      _ptr(out_f16, torch.float16, "out_f16"), _stream()), "rtxn_ema_weights")


def volrender_scaled_train(network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, scaler, pixels,
                           loss_gradients, loss_sum, radiance_gradients, background=None, loss=None, regularizer=None):
    """rtxn_volrender_scaled_train: volrender_reg_train reading the loss scale from the scaler's device word; always the loss
    compositor's kernels, plain L2 included."""
    _composite_train("volrender_scaled_train", (network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, 0.0,
                                                pixels, loss_gradients, loss_sum, radiance_gradients), (background, loss, regularizer, scaler))


def deterministic_shadow(n_params, device="cuda"):
    """A zeroed 64-bit fixed-point shadow for a gradient buffer of n_params floats (rtxn_deterministic_workspace_bytes)."""
    nbytes = _lib.lib().rtxn_deterministic_workspace_bytes(int(n_params))
    return torch.zeros(nbytes // 8, dtype=torch.int64, device=device)


# the shadows the library holds pointers to: kept alive here until the next set_deterministic call replaces them
_det_registered = (None, None)


def set_deterministic(mlp_shadow=None, table_shadow=None):
    """rtxn_set_deterministic_workspace: process-wide; (None, None) restores the float atomics.  The tensors stay referenced
    here until the next call, so the library never holds a pointer into freed memory."""
    global _det_registered
    check(_lib.lib().rtxn_set_deterministic_workspace(_ptr(mlp_shadow, torch.int64, "mlp_shadow"), _ptr(table_shadow, torch.int64, "table_shadow")),
          "rtxn_set_deterministic_workspace")
    _det_registered = (mlp_shadow, table_shadow)


def release_deterministic(mlp_shadow, table_shadow):
    """Restore the float atomics (set_deterministic(None, None)) if exactly these shadows are the registered ones; otherwise
    leave the selection alone.  What a deterministic Trainer runs when it is finalized."""
    m, t = _det_registered
    if m is mlp_shadow and t is table_shadow and (m is not None or t is not None):
        set_deterministic(None, None)


def train_gradients(net, *, grid=None, n_dir_freqs=0, table=None, start_points, end_points, seg_view, num_stored, indices,
                    total_segments, segment_capacity, n_rays, sample_type, t_scale=1.0, vr_mode, targets, loss_scale,
                    encT, dencT=None, workspace=None, output_half, radiance, t_vals, radiance_gradients, pixels, loss_gradients,
                    loss_sum=None, dparams, dtable=None, dtable_hashed_half=None, live_ws=None, skip_table_backward=False,
                    workspace_lean=False, background=None, jitter=None, loss=None, regularizer=None, scaler=None, rays=None, depth=None):
    """rtxn_train_gradients: sampler ... backward of one batch with the segment count taken on the device (main.cu:703-781).
    rays: ray_gradients(...) -> rtxn_train_gradients_rays (with or without any of the five below): dL/d(rays_o), dL/d(rays_d)
    behind the table scatter; its t_start / t_end must already hold the batch's distances (trace_grid, TRACE_DDA).
    background: train_background(...) -> rtxn_train_gradients_ex (targets float[n_rays][background.target_channels]);
    jitter: sample_jitter(...) with SAMPLING_JITTER_WORLD -> rtxn_train_gradients_jitter (with or without a background);
    loss: train_loss(...) -> rtxn_train_gradients_loss (with or without either);
    regularizer: train_regularizer(...) -> rtxn_train_gradients_reg (with or without any of the three);
    scaler: loss_scaler(...) -> rtxn_train_gradients_scaled (with or without any of the four; loss_scale is then not read);
    depth: train_depth(...) -> rtxn_train_gradients_depth (with or without any of the six)."""
    kw = {k: v for k, v in locals().items() if k not in ("background", "jitter", "regularizer", "scaler", "rays", "depth")}
    _check_regularizer("train_gradients", regularizer, n_rays, segment_capacity)
    _check_depth("train_gradients", depth, n_rays, segment_capacity)
    _check_ray_gradients("train_gradients", rays, n_rays, segment_capacity)
    b = train_batch(**kw, target_channels=background.target_channels if background is not None else 3)
    options = (background, jitter, loss, regularizer, scaler, rays, depth)
    name, n_options = _ladder_entry("rtxn_train_gradients", _GRADIENTS_LADDER, options)
    check(getattr(_lib.lib(), name)(C.byref(b), *map(_byref, options[:n_options]), _stream()), name)


# The rungs of the step and gradients ladders (include/rtxn.h), topmost first: (suffix, how many of the options
# (background, jitter, loss, regularizer, ...) the rung takes, which of them select it).  The call goes to the topmost rung one of
# whose own options is given: the lowest entry point that takes everything that is.
_STEP_LADDER = (("_depth", 11, (10,)), ("_cameras", 10, (9,)), ("_rays", 9, (7, 8)), ("_ema", 7, (6,)), ("_scaled", 6, (5,)), ("_opt", 5, (4,)), ("_reg", 4, (3,)), ("_loss", 3, (2,)),
                ("_jitter", 2, (1,)), ("_ex", 1, (0,)), ("", 0, ()))
_GRADIENTS_LADDER = (("_depth", 7, (6,)), ("_rays", 6, (5,)), ("_scaled", 5, (4,)), ("_reg", 4, (3,)), ("_loss", 3, (2,)), ("_jitter", 2, (1,)), ("_ex", 1, (0,)),
                     ("", 0, ()))


def _ladder_entry(prefix, ladder, options):
    for suffix, n_options, own in ladder:
        if not own or any(i < len(options) and options[i] is not None for i in own):      # a shorter tuple: the rungs it reaches
            return prefix + suffix, n_options


def train_batch(net, *, grid=None, n_dir_freqs=0, table=None, start_points, end_points, seg_view, num_stored, indices,
                total_segments, segment_capacity, n_rays, sample_type, t_scale=1.0, vr_mode, targets, loss_scale,
                encT, dencT=None, workspace=None, output_half, radiance, t_vals, radiance_gradients, pixels, loss_gradients,
                loss_sum=None, dparams, dtable=None, dtable_hashed_half=None, live_ws=None, skip_table_backward=False,
                workspace_lean=False, target_channels=3, loss=None):
    """struct rtxn_train_batch over the given tensors (which the caller keeps alive), sizes checked against the capacity
    (targets: target_channels floats per ray).  loss: the train_loss(...) the batch will be stepped with -- not part of the
    struct, its opacity buffer is sized against n_rays here."""
    if loss is not None and loss.opacity and loss._opacity_tensor.numel() < int(n_rays):
        raise _lib.RtxnError(f"train_gradients: loss.opacity holds {loss._opacity_tensor.numel()} elements, {n_rays} rays")
    b = _lib.TrainBatch()
    b.mlp, b.grid = net._h, (grid._h if grid is not None else None)
    b.n_dir_freqs = int(n_dir_freqs)
    b.table_fp16 = _ptr(table, torch.float16, "table")
    b.start_points, b.end_points = _ptr(start_points, torch.float32, "start_points"), _ptr(end_points, torch.float32, "end_points")
    b.seg_view = _ptr(seg_view, torch.float32, "seg_view")
    b.num_stored, b.indices = _ptr(num_stored, torch.int32, "num_stored"), _ptr(indices, torch.int32, "indices")
    b.total_segments = _ptr(total_segments, torch.int32, "total_segments")
    b.segment_capacity, b.n_rays, b.sample_type, b.t_scale, b.vr_mode = int(segment_capacity), int(n_rays), int(sample_type), float(t_scale), int(vr_mode)
    b.targets, b.loss_scale = _ptr(targets, torch.float32, "targets"), float(loss_scale)
    b.encT, b.dencT = _ptr(encT, torch.float16, "encT"), _ptr(dencT, torch.float16, "dencT")
    b.workspace = _ptr(workspace, torch.float16, "workspace")
    b.output_half, b.radiance = _ptr(output_half, torch.float16, "output_half"), _ptr(radiance, torch.float32, "radiance")
    b.t_vals, b.radiance_gradients = _ptr(t_vals, torch.float32, "t_vals"), _ptr(radiance_gradients, torch.float16, "radiance_gradients")
    b.pixels, b.loss_gradients_half = _ptr(pixels, torch.float32, "pixels"), _ptr(loss_gradients, torch.float16, "loss_gradients")
    b.loss_sum = _ptr(loss_sum, torch.float32, "loss_sum")
    b.dparams, b.dtable = _ptr(dparams, torch.float32, "dparams"), _ptr(dtable, torch.float32, "dtable")
    b.dtable_hashed_half = _ptr(dtable_hashed_half, torch.float16, "dtable_hashed_half")
    if live_ws is not None and live_ws.numel() * live_ws.element_size() < live_segments_workspace_bytes(segment_capacity):
        raise _lib.RtxnError("train_gradients: live_ws smaller than live_segments_workspace_bytes(segment_capacity)")
    b.live_ws = _ptr(live_ws, None, "live_ws")
    b.skip_table_backward = 1 if skip_table_backward else 0
    b.workspace_lean = 1 if workspace_lean else 0
    for nm, t, need in (("encT", encT, net.encoded_width() * padded_samples(32 * int(segment_capacity))),
                        ("output_half", output_half, 32 * int(segment_capacity) * 16), ("radiance", radiance, 32 * int(segment_capacity) * 4),
                        ("t_vals", t_vals, 32 * int(segment_capacity)), ("radiance_gradients", radiance_gradients, 32 * int(segment_capacity) * 4),
                        ("start_points", start_points, 3 * int(segment_capacity)), ("end_points", end_points, 3 * int(segment_capacity)),
                        ("seg_view", seg_view, 2 * int(segment_capacity)), ("pixels", pixels, 3 * int(n_rays)),
                        ("targets", targets, int(target_channels) * int(n_rays)), ("num_stored", num_stored, int(n_rays)), ("indices", indices, int(n_rays))):
        if t.numel() < need:
            raise _lib.RtxnError(f"train_gradients: {nm} holds {t.numel()} elements, {need} needed for capacity {segment_capacity} / {n_rays} rays")
    return b


def train_step(args, background=None, jitter=None, loss=None, regularizer=None, optimizer=None, scaler=None, ema=None, rays=None, pose=None,
               cameras=None, depth=None):
    """rtxn_train_step(args: _lib.TrainStepArgs): traversal -> gradients -> optimizer of one batch, one call, current stream.
    background: train_background(...) -> rtxn_train_step_ex (RANDOM with step None hashes args.opt.step before the increment);
    jitter: sample_jitter(...) -> rtxn_train_step_jitter (step None: args.opt.step, by the same rule);
    loss: train_loss(...) -> rtxn_train_step_loss (with or without either);
    regularizer: train_regularizer(...) -> rtxn_train_step_reg (with or without any of the three): the write pass of the traversal
    stores the segments' t_start / t_end into the regulariser's buffers;
    optimizer: optimizer_options(...) -> rtxn_train_step_opt (with or without any of the four);
    scaler: loss_scaler(...) -> rtxn_train_step_scaled (needs `optimizer` with skip_nonfinite);
    ema: weight_ema(...) -> rtxn_train_step_ema (needs `optimizer`, which may have nothing switched on; with or without a scaler);
    rays: ray_gradients(...), pose: pose_refinement(...) -> rtxn_train_step_rays (with or without any of the seven; pose needs rays):
    the write pass stores t_start / t_end into rays' buffers, the ray gradients are formed behind the table scatter and the pose
    gradient and step run behind the optimizer;
    cameras: camera_refinement(...) with drawn and poses -> rtxn_train_step_cameras (needs rays): behind the optimizer the pose
    gradient, the camera gradient, the pose step, the camera step;
    depth: train_depth(...) -> rtxn_train_step_depth (with or without any of the ten): the write pass stores t_start / t_end into
    its buffers, the compositor adds the depth term."""
    _check_regularizer("train_step", regularizer, args.batch.n_rays, args.batch.segment_capacity)
    _check_depth("train_step", depth, args.batch.n_rays, args.batch.segment_capacity)
    _check_ray_gradients("train_step", rays, args.batch.n_rays, args.batch.segment_capacity)
    terms = getattr(cameras, "_tensors", {}).get("terms")
    if terms is not None and terms.numel() < 12 * int(args.batch.n_rays):
        raise _lib.RtxnError(f"train_step: cameras.terms holds {terms.numel()} elements, {12 * int(args.batch.n_rays)} needed")
    options = (background, jitter, loss, regularizer, optimizer, scaler, ema, rays, pose, cameras, depth)
    name, n_options = _ladder_entry("rtxn_train_step", _STEP_LADDER, options)
    check(getattr(_lib.lib(), name)(C.byref(args), *map(_byref, options[:n_options]), _stream()), name)


def half2_workspace(values, block_entries):
    """int32 workspace of rtxn_half2_count_nonzero / _pack_nonzero for `values` (fp16, two halves per entry)."""
    nbytes = int(_lib.lib().rtxn_half2_workspace_bytes(values.numel() // 2, int(block_entries)))
    return torch.zeros(nbytes // 4, dtype=torch.int32, device=values.device)


def half2_count_nonzero(values, block_entries, workspace=None):
    """rtxn_half2_count_nonzero: non-zero half2 entries per block of `values` -> workspace (its first `blocks` ints are the
    per-block counts; returns (counts view, workspace))."""
    n = values.numel() // 2
    nb = (n + block_entries - 1) // block_entries
    if workspace is None:
        workspace = half2_workspace(values, block_entries)
    check(_lib.lib().rtxn_half2_count_nonzero(_ptr(values, torch.float16, "values"), n, int(block_entries),
                                              _ptr(workspace, torch.int32, "workspace"), _stream()), "rtxn_half2_count_nonzero")
    return workspace[:nb], workspace


def half2_pack_nonzero(values, block_entries, workspace, block_mask, pairs, count, clear=True):
    """rtxn_half2_pack_nonzero: (index, half2 bits) of the non-zero entries of the masked blocks, ascending -> pairs
    int32[capacity][2]; count (device int32[1]) = entries needed.  workspace: as half2_count_nonzero left it for these values."""
    need = int(_lib.lib().rtxn_half2_workspace_bytes(values.numel() // 2, int(block_entries)))
    if workspace.numel() * 4 < need:
        raise _lib.RtxnError(f"half2_pack_nonzero: workspace of {workspace.numel() * 4} bytes, {need} needed")
    check(_lib.lib().rtxn_half2_pack_nonzero(_ptr(values, torch.float16, "values"), values.numel() // 2, int(block_entries),
                                             _ptr(workspace, torch.int32, "workspace"), int(block_mask), pairs.numel() // 2,
                                             _ptr(pairs, torch.int32, "pairs"), _ptr(count, torch.int32, "count"),
                                             1 if clear else 0, _stream()), "rtxn_half2_pack_nonzero")


def half2_add_pairs(values, pairs, count):
    """rtxn_half2_add_pairs: values[index] += value over the first `count` pairs of one list."""
    if count > pairs.numel() // 2:
        raise _lib.RtxnError(f"half2_add_pairs: count {count} > {pairs.numel() // 2} pairs held")
    check(_lib.lib().rtxn_half2_add_pairs(_ptr(values, torch.float16, "values"), values.numel() // 2, _ptr(pairs, torch.int32, "pairs"),
                                          int(count), _stream()), "rtxn_half2_add_pairs")


def live_segments_workspace_bytes(segment_capacity):
    return int(_lib.lib().rtxn_live_segments_workspace_bytes(int(segment_capacity)))


def live_segments_workspace(segment_capacity, device="cuda"):
    """[int count | pad | int list[capacity] | flags]: see rtxn_live_segments (include/rtxn.h)."""
    return torch.zeros((live_segments_workspace_bytes(segment_capacity) + 3) // 4, dtype=torch.int32, device=device)


def live_segments(radiance_gradients, n_segments, segment_capacity, live_ws):
    """List the 32-sample segments whose radiance gradient is not all zero; count = live_ws[0], list = live_ws[4:4+count]."""
    check(_lib.lib().rtxn_live_segments(_ptr(radiance_gradients, torch.float16, "radiance_gradients"), int(n_segments),
                                        int(segment_capacity), _ptr(live_ws, None, "live_ws"), _stream()), "rtxn_live_segments")


def convert_f32_to_f16(src, dst):
    check(_lib.lib().rtxn_convert_f32_to_f16(_ptr(src, torch.float32, "src"), _ptr(dst, torch.float16, "dst"), src.numel(), _stream()),
          "rtxn_convert_f32_to_f16")


def convert_f16_to_f32(src, dst):
    check(_lib.lib().rtxn_convert_f16_to_f32(_ptr(src, torch.float16, "src"), _ptr(dst, torch.float32, "dst"), src.numel(), _stream()),
          "rtxn_convert_f16_to_f32")


# --------------------------------------------------------------------------- device batches
IMAGE_F32, IMAGE_U8 = 0, 1                 # enum rtxn_image_format
DEPTH_U16, DEPTH_F32 = 0, 1                # enum rtxn_depth_format
DEPTH_Z, DEPTH_RAY = 0, 1                  # enum rtxn_depth_kind
DEPTH_KINDS = {"z": DEPTH_Z, "ray": DEPTH_RAY}
WORLD_ORIGIN_SCALE = 0.1                   # o_k = la[4k+3] / 10 (rtxn_draw_batch): a pose-unit length in world units


class ImageSet:
    """struct rtxn_image_set (include/rtxn.h) over resident training frames: `images` a device tensor [N, H, W, C] (C = 3 or 4),
    float32 or uint8 (v / 255 on read), `poses` [N, 16] or [N, 4, 4] float32 on the same device, one pinhole camera
    (focal_length and aspect_ratio as rtxn_trace_params; aspect_ratio defaults to W / H) for all of them.  A thin holder: it keeps the two tensors
    alive and hands draw_batch() their pointers.  cameras: a CameraSet (camera_set()) of 1 or N cameras on the images' device,
    kept alive here; batches drawn from the set and frames evaluated against it then take their rays from it, and focal_length
    may be omitted (it is not read).  depth: per-pixel depth maps, a device tensor [N, H, W], uint16 or float32, on the images'
    device, in units of depth_unit world-before-origin-scale lengths (the poses' unit); 0 = no measurement.  depth_kind "z": the
    distance along the optical axis (the usual depth map), "ray": along the pixel's ray.  Kept alive here for depth_targets()."""

    def __init__(self, images, poses, focal_length=None, aspect_ratio=None, cameras=None, depth=None, depth_unit=1.0, depth_kind="z"):
        if images.dim() != 4 or images.shape[-1] not in (3, 4) or images.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"ImageSet: images of shape {tuple(images.shape)} / {images.dtype}: [N, H, W, 3 | 4], float32 or uint8")
        n, h, w, c = (int(v) for v in images.shape)
        if n < 1 or h < 1 or w < 1 or w * h > 1 << 24:
            raise ValueError(f"ImageSet: {n} frames of {w} x {h}: at least one frame, width * height <= 1 << 24")
        if poses.dtype != torch.float32 or poses.numel() != 16 * n or tuple(poses.shape[1:]) not in ((16,), (4, 4)):
            raise ValueError(f"ImageSet: poses of shape {tuple(poses.shape)} / {poses.dtype}: float32 [{n}, 16] or [{n}, 4, 4]")
        if poses.device != images.device:
            raise ValueError(f"ImageSet: images on {images.device}, poses on {poses.device}")
        if cameras is None and focal_length is None:
            raise ValueError("ImageSet: focal_length is required without cameras")
        if cameras is not None:
            if not isinstance(cameras, CameraSet) or cameras.n_cameras not in (1, n):
                raise ValueError(f"ImageSet: cameras must be a CameraSet of 1 or {n} cameras")
            if cameras.params.device != images.device:
                raise ValueError(f"ImageSet: images on {images.device}, cameras on {cameras.params.device}")
            cameras.check_invertible(w, h)
        self.images, self.poses = images.contiguous(), poses.reshape(n, 16).contiguous()
        self.n_images, self.height, self.width, self.channels = n, h, w, c
        self.format = IMAGE_U8 if images.dtype == torch.uint8 else IMAGE_F32
        self.cameras = cameras
        if depth is not None:
            if tuple(depth.shape) != (n, h, w) or depth.dtype not in (torch.uint16, torch.float32):
                raise ValueError(f"ImageSet: depth of shape {tuple(depth.shape)} / {depth.dtype}: [{n}, {h}, {w}], uint16 or float32")
            if depth.device != images.device:
                raise ValueError(f"ImageSet: images on {images.device}, depth on {depth.device}")
            if depth_kind not in DEPTH_KINDS:
                raise ValueError(f"ImageSet: depth_kind {depth_kind!r}: one of {sorted(DEPTH_KINDS)}")
            if not (float(depth_unit) > 0.0 and float(depth_unit) < float("inf")):
                raise ValueError(f"ImageSet: depth_unit = {depth_unit} (finite, > 0)")
            depth = depth.contiguous()
        self.depth, self.depth_unit, self.depth_kind = depth, float(depth_unit), depth_kind
        self.focal_length = None if focal_length is None else float(focal_length)
        self.aspect_ratio = float(aspect_ratio) if aspect_ratio is not None else w / h

    @classmethod
    def from_dataset(cls, dataset, corrected_focal=True, storage="u8", device="cuda", cameras=None, depth=None, depth_unit=1.0,
                     depth_kind="z"):
        """dataset: rtx_nerf_amd.loader.ImageDataset; the focal rule is RayDataset.from_images' (corrected_focal:
        1/tan(camera_angle_x/2) instead of the reference's 1/tan(0.5*focal_px), quirk Q1).  storage "f32" keeps the loader's
        floats; "u8" quantises them ONCE on the host with round(v * 255) -- a quarter of the memory, and exact (the drawn
        v / 255 is the loader's float, bit for bit) for datasets loaded with flags bit 1 (v / 255, no gamma), whose values are
        k / 255 already; gamma-linearised frames (flags 0) are rounded to the nearest 1/255.  cameras: as ImageSet's.  depth: a numpy array
        or tensor [N, H, W], uint16 or float32 (loader.read_depth_maps), moved to `device`; depth_unit, depth_kind: as ImageSet's.
        Returns (image_set, focal)."""
        import math
        import numpy as np
        if storage not in ("u8", "f32"):
            raise ValueError(f"ImageSet.from_dataset: storage {storage!r} (u8 | f32)")
        if corrected_focal:
            focal = 1.0 / math.tan(0.5 * dataset.camera_angle_x)
        else:
            focal = float(np.float32(1.0) / np.tan(np.float32(0.5) * np.float32(dataset.focal)))
        W, H = int(dataset.image_width), int(dataset.image_height)
        ch = int(dataset.image_channels) or 3
        img = np.ascontiguousarray(dataset.images, dtype=np.float32).reshape(-1, H, W, ch)
        if storage == "u8":
            img = np.clip(np.rint(img * np.float32(255.0)), 0, 255).astype(np.uint8)
        poses = np.ascontiguousarray(dataset.poses, dtype=np.float32).reshape(-1, 16)
        if depth is not None:
            depth = (depth if isinstance(depth, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(depth))).to(device)
        return cls(torch.from_numpy(img).to(device), torch.from_numpy(poses).to(device), focal, cameras=cameras, depth=depth,
                   depth_unit=depth_unit, depth_kind=depth_kind), focal

    def nbytes(self):
        """bytes held on the device"""
        return (self.images.numel() * self.images.element_size() + self.poses.numel() * 4 +
                (self.depth.numel() * self.depth.element_size() if self.depth is not None else 0))

    def c_struct(self):
        s = _lib.ImageSet()
        s.images, s.poses = _ptr(self.images, name="images"), _ptr(self.poses, torch.float32, "poses")
        s.n_images, s.width, s.height, s.channels, s.format = self.n_images, self.width, self.height, self.channels, self.format
        s.focal_length, s.aspect_ratio = (0.0 if self.focal_length is None else self.focal_length), self.aspect_ratio
        return s

    def camera_of(self, image):
        """the index into self.cameras of frame `image`"""
        return 0 if self.cameras.n_cameras == 1 else int(image)


def draw_batch_args(image_set, n, seed, step, rays_o, rays_d, targets, drawn=None, cameras=None):
    """struct rtxn_draw_batch_args over the given tensors (which the caller keeps alive): rays_o, rays_d float32 [>= n, 3],
    targets float32 [>= n, channels], drawn int32 [>= n, 2] or None, step a device int32 tensor or None (0).  cameras: a
    CameraSet, default the image set's own (None: the set's pinhole); the struct keeps it, and draw_batch_launch() then draws
    through rtxn_draw_batch_cameras."""
    n, C_ = int(n), image_set.channels
    for t, w, nm in ((rays_o, 3, "rays_o"), (rays_d, 3, "rays_d"), (targets, C_, "targets"), (drawn, 2, "drawn")):
        if t is not None and (t.dim() != 2 or t.shape[1] != w or t.shape[0] < n):
            raise _lib.RtxnError(f"draw_batch: {nm} of shape {tuple(t.shape)}: [>= {n}, {w}]")
    a = _lib.DrawBatchArgs()
    a.set = image_set.c_struct()
    a.n_rays, a.seed = n, int(seed) & 0xFFFFFFFF
    a.step = _ptr(step, torch.int32, "step")
    a.rays_o, a.rays_d = _ptr(rays_o, torch.float32, "rays_o"), _ptr(rays_d, torch.float32, "rays_d")
    a.targets = _ptr(targets, torch.float32, "targets")
    a.drawn = _ptr(drawn, torch.int32, "drawn")
    cameras = image_set.cameras if cameras is None else cameras
    if cameras is not None and cameras is not image_set.cameras:
        cameras.check_invertible(image_set.width, image_set.height)
    a._cameras = cameras
    a._camera_struct = cameras.c_struct() if cameras is not None else None
    return a


def draw_batch(image_set, n, seed, step, rays_o, rays_d, targets, drawn=None, cameras=None):
    """rtxn_draw_batch: batch number `step` (device int32 tensor, None: 0) of the sequence `seed` keys, n rays drawn from
    image_set into rays_o / rays_d / targets on the current stream; drawn (int32 [n, 2], optional) receives (image, y*W + x).
    With cameras (a CameraSet; default the image set's own) rtxn_draw_batch_cameras: the same (image, pixel) and target bits, the
    ray from image's camera."""
    draw_batch_launch(draw_batch_args(image_set, n, seed, step, rays_o, rays_d, targets, drawn, cameras))


def depth_targets_args(image_set, n, drawn, rays_d, target):
    """struct rtxn_depth_targets_args over the set's depth maps and LIVE poses and the given tensors (which the caller keeps alive):
    drawn int32 [>= n, 2] as draw_batch() recorded it, rays_d float32 [>= n, 3], target float32 [>= n].  scale = the set's
    depth_unit times the world's origin scale, formed here once, in float32."""
    import numpy as np
    if image_set.depth is None:
        raise _lib.RtxnError("depth_targets: the image set holds no depth maps (ImageSet(..., depth=...))")
    n = int(n)
    for t, w, nm in ((drawn, 2, "drawn"), (rays_d, 3, "rays_d")):
        if t is None or t.dim() != 2 or t.shape[1] != w or t.shape[0] < n:
            raise _lib.RtxnError(f"depth_targets: {nm} of shape {None if t is None else tuple(t.shape)}: [>= {n}, {w}]")
    if target is None or target.numel() < n:
        raise _lib.RtxnError(f"depth_targets: target holds {0 if target is None else target.numel()} elements, {n} rays")
    a = _lib.DepthTargetsArgs()
    a.depth, a.poses = _ptr(image_set.depth, name="depth"), _ptr(image_set.poses, torch.float32, "poses")
    a.n_images, a.width, a.height = image_set.n_images, image_set.width, image_set.height
    a.format = DEPTH_U16 if image_set.depth.dtype == torch.uint16 else DEPTH_F32
    a.kind = DEPTH_KINDS[image_set.depth_kind]
    a.scale = float(np.float32(image_set.depth_unit) * np.float32(WORLD_ORIGIN_SCALE))
    a.n_rays = n
    a.drawn, a.rays_d = _ptr(drawn, torch.int32, "drawn"), _ptr(rays_d, torch.float32, "rays_d")
    a.target = _ptr(target, torch.float32, "target")
    return a


def depth_targets(image_set, n, drawn, rays_d, target):
    """rtxn_depth_targets: the depth targets of a drawn batch (distances along the rays, world units; 0 = no target) from the set's
    depth maps, on the current stream, right behind draw_batch()."""
    depth_targets_launch(depth_targets_args(image_set, n, drawn, rays_d, target))


def depth_targets_launch(args):
    """rtxn_depth_targets over a struct depth_targets_args() built earlier (its tensors still alive), on the current stream."""
    check(_lib.lib().rtxn_depth_targets(C.byref(args), _stream()), "rtxn_depth_targets")


def draw_batch_launch(args):
    """rtxn_draw_batch[_cameras] over a struct draw_batch_args() built earlier (its tensors still alive), on the current stream."""
    cams = getattr(args, "_camera_struct", None)
    if cams is not None:
        check(_lib.lib().rtxn_draw_batch_cameras(C.byref(args), C.byref(cams), _stream()), "rtxn_draw_batch_cameras")
    else:
        check(_lib.lib().rtxn_draw_batch(C.byref(args), _stream()), "rtxn_draw_batch")


# --------------------------------------------------------------------------- camera models
CAMERA_PINHOLE, CAMERA_OPENCV, CAMERA_OPENCV_FISHEYE = 0, 1, 2      # enum rtxn_camera_model
CAMERA_MODELS = {"pinhole": CAMERA_PINHOLE, "opencv": CAMERA_OPENCV, "opencv_fisheye": CAMERA_OPENCV_FISHEYE}
CAMERA_PARAMS = 12


def camera_params(fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, k4=0.0, p1=0.0, p2=0.0):
    """One camera's row of twelve floats: fx, fy, cx, cy in pixels, then k1, k2, k3, k4, p1, p2, 0, 0 (include/rtxn.h)."""
    return [float(fx), float(fy), float(cx), float(cy), float(k1), float(k2), float(k3), float(k4), float(p1), float(p2), 0.0, 0.0]


def _camera_residual(model, P, xd, yd):
    """Host float64: the Newton solve of the device function run to convergence (50 iterations) for the rows P [n, 12] at the
    distorted positions xd, yd [n, m].  Returns (residual, det) [n, m]: |distort(solution) - (xd, yd)|_inf and the Jacobian
    determinant (fisheye: the derivative) at the solution."""
    k1, k2, k3, k4, p1, p2 = (P[:, i:i + 1] for i in (4, 5, 6, 7, 8, 9))
    with np.errstate(all="ignore"):
        if model == CAMERA_OPENCV:
            def f(x, y):
                r2 = x * x + y * y
                rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
                drad = k1 + r2 * (2 * k2 + r2 * 3 * k3)
                fx_ = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) - xd
                fy_ = y * rad + 2 * p2 * x * y + p1 * (r2 + 2 * y * y) - yd
                j11 = rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
                j22 = rad + 2 * y * y * drad + 2 * p2 * x + 6 * p1 * y
                j12 = 2 * x * y * drad + 2 * (p1 * x + p2 * y)
                return fx_, fy_, j11, j12, j22
            x, y = xd.copy(), yd.copy()
            for _ in range(50):
                fx_, fy_, j11, j12, j22 = f(x, y)
                det = j11 * j22 - j12 * j12
                ok = np.isfinite(det) & (det != 0)
                safe = np.where(ok, det, 1.0)
                x = np.where(ok, x - (j22 * fx_ - j12 * fy_) / safe, x)
                y = np.where(ok, y - (j11 * fy_ - j12 * fx_) / safe, y)
            fx_, fy_, j11, j12, j22 = f(x, y)
            return np.maximum(np.abs(fx_), np.abs(fy_)), j11 * j22 - j12 * j12
        thd = np.hypot(xd, yd)

        def g(th):
            t2 = th * th
            poly = 1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
            dpoly = 1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4)))
            return th * poly - thd, dpoly
        th = thd.copy()
        for _ in range(50):
            f_, d_ = g(th)
            ok = np.isfinite(d_) & (d_ != 0)
            th = np.where(ok, th - f_ / np.where(ok, d_, 1.0), th)
        f_, d_ = g(th)
        return np.abs(f_), d_


class CameraSet:
    """struct rtxn_camera_set (include/rtxn.h) over a float32 [n, 12] tensor of camera rows (camera_params()): one model for
    the set, n = 1 (shared by every image) or one camera per image.  A thin holder: it keeps the tensor alive and hands the
    library its pointer.  Build it with camera_set()."""

    def __init__(self, model, params):
        self.model, self.params = int(model), params
        self.n_cameras = int(params.shape[0])
        self._host = params.detach().cpu().numpy().astype(np.float64)
        self._checked = set()

    def check_invertible(self, width, height):
        """ValueError unless every camera of the set is invertible over a width x height frame: on the host, in float64, at a
        33 x 33 lattice of pixel positions spanning the frame's corners ([0, width] x [0, height]) the Newton solve of the device
        function, run to convergence, must reproduce the position (residual <= 1e-9) with a positive Jacobian determinant at
        the solution.  Uses the host copy of the parameters: as they were when the set was built, or at the last refresh_host()."""
        key = (int(width), int(height))
        if key in self._checked:
            return
        P = self._host
        bad = ~(np.isfinite(P).all(1) & (P[:, 0] > 0) & (P[:, 1] > 0))
        if bad.any():
            c = int(np.argmax(bad))
            raise ValueError(f"camera_set: camera {c}: fx = {P[c, 0]}, fy = {P[c, 1]} must be positive and every parameter finite")
        if self.model != CAMERA_PINHOLE:
            px, py = np.meshgrid(np.linspace(0.0, float(width), 33), np.linspace(0.0, float(height), 33))
            px, py = px.reshape(1, -1), py.reshape(1, -1)
            xd, yd = (px - P[:, 2:3]) / P[:, 0:1], (py - P[:, 3:4]) / P[:, 1:2]
            res, det = _camera_residual(self.model, P, xd, yd)
            bad = ~((res <= 1e-9) & (det > 0))
            if bad.any():
                c, j = (int(v) for v in np.argwhere(bad)[0])
                name = [k for k, v in CAMERA_MODELS.items() if v == self.model][0]
                raise ValueError(f"camera_set: camera {c} ({name}) is not invertible over the {width} x {height} frame: at pixel "
                                 f"({px[0, j]:.2f}, {py[0, j]:.2f}) the float64 solve leaves a residual of {res[c, j]:.3g} with "
                                 f"Jacobian determinant {det[c, j]:.3g}")
        self._checked.add(key)

    def refresh_host(self):
        """Read the rows back from the device (they may have been refined in place: Trainer.attach_images(refine_cameras=)) and
        forget every frame size checked so far, so that the next check_invertible() judges the live parameters."""
        self._host = self.params.detach().cpu().numpy().astype(np.float64)
        self._checked = set()
        return self

    def c_struct(self):
        s = _lib.CameraSet()
        s.model, s.n_cameras = self.model, self.n_cameras
        s.params = _ptr(self.params, torch.float32, "camera params")
        return s


def camera_set(model, params, width=None, height=None, device="cuda"):
    """A CameraSet: model "pinhole" | "opencv" | "opencv_fisheye"; params a float32 [n, 12] (or [12]) array or tensor of
    camera_params() rows, moved to `device`.
    DOMAIN.  The device function has no per-ray validity flag: it runs 8 Newton steps whatever they do.  So parameters that are
    not invertible over the frame are refused here, on the host (CameraSet.check_invertible: a 33 x 33 lattice over
    [0, width] x [0, height]; ValueError naming the camera and the pixel).  width, height: the frame; without them the frame
    is taken as [0, 2 cx] x [0, 2 cy] per camera (a principal point at the centre), and api.ImageSet(cameras=) checks again
    with its own size.  Pixels outside the checked frame are outside the contract."""
    if model not in CAMERA_MODELS:
        raise ValueError(f"camera_set: model {model!r}: one of {sorted(CAMERA_MODELS)}")
    t = torch.as_tensor(np.asarray(params.detach().cpu() if isinstance(params, torch.Tensor) else params, dtype=np.float32))
    if t.dim() == 1:
        t = t.reshape(1, -1)
    if t.dim() != 2 or t.shape[1] != CAMERA_PARAMS or t.shape[0] < 1:
        raise ValueError(f"camera_set: params of shape {tuple(t.shape)}: [n, {CAMERA_PARAMS}] or [{CAMERA_PARAMS}]")
    cs = CameraSet(CAMERA_MODELS[model], t.contiguous().to(device))
    if width is not None and height is not None:
        cs.check_invertible(width, height)
    else:
        for c in range(cs.n_cameras):
            one = CameraSet(cs.model, t[c:c + 1])
            try:
                one.check_invertible(2.0 * float(t[c, 2]), 2.0 * float(t[c, 3]))
            except ValueError as e:
                raise ValueError(str(e).replace("camera 0", f"camera {c}", 1)) from None
    return cs


def camera_set_check(cameras, n_images):
    """rtxn_camera_set_check: the library's own rules (model, n_cameras in {1, n_images}, params), host only."""
    s = cameras.c_struct() if isinstance(cameras, CameraSet) else cameras
    check(_lib.lib().rtxn_camera_set_check(C.byref(s), int(n_images)), "rtxn_camera_set_check")


def camera_rays(cameras, camera, look_at, width, height, ray_begin=0, ray_count=None, rays_o=None, rays_d=None):
    """rtxn_camera_rays: the rays of launch pixels [ray_begin, ray_begin + ray_count) of a width x height frame of camera
    `camera` under look_at (16 device floats), written at their launch index into rays_o / rays_d (float32 [width*height, 3];
    new ones when None -- elements outside the window are then uninitialised).  One kernel on the current stream.
    Returns (rays_o, rays_d)."""
    n = int(width) * int(height)
    if look_at.numel() != 16:
        raise _lib.RtxnError(f"camera_rays: look_at of shape {tuple(look_at.shape)}: 16 floats")
    if rays_o is None:
        rays_o = torch.empty((n, 3), device=look_at.device)
    if rays_d is None:
        rays_d = torch.empty((n, 3), device=look_at.device)
    for t, nm in ((rays_o, "rays_o"), (rays_d, "rays_d")):
        if t.numel() < 3 * n:
            raise _lib.RtxnError(f"camera_rays: {nm} of shape {tuple(t.shape)}: [{n}, 3]")
    s = cameras.c_struct()
    check(_lib.lib().rtxn_camera_rays(C.byref(s), int(camera), _ptr(look_at, torch.float32, "look_at"), int(width), int(height),
                                      int(ray_begin), n - int(ray_begin) if ray_count is None else int(ray_count),
                                      _ptr(rays_o, torch.float32, "rays_o"), _ptr(rays_d, torch.float32, "rays_d"), _stream()),
          "rtxn_camera_rays")
    return rays_o, rays_d


# --------------------------------------------------------------------------- held-out evaluation
METRICS_SSIM, METRICS_CLAMP = 1, 2         # enum rtxn_metrics_flags


def image_metrics_workspace_bytes(width, height):
    """rtxn_image_metrics_workspace_bytes: the bytes of partial sums rtxn_image_metrics needs for width x height frames."""
    lib = _lib.lib()
    need = lib.rtxn_image_metrics_workspace_bytes(int(width), int(height))
    if need == 0:
        msg = lib.rtxn_last_error()
        raise _lib.RtxnError(f"rtxn_image_metrics_workspace_bytes: {msg.decode() if msg else '?'}")
    return int(need)


def image_metrics_workspace(image_set):
    """A workspace for image_metrics() over image_set's frames, on the set's device (uint8, from an 8-byte aligned allocation)."""
    return torch.empty(image_metrics_workspace_bytes(image_set.width, image_set.height), dtype=torch.uint8, device=image_set.images.device)


def image_metrics_args(image_set, image, pred, *, background=None, ssim=True, clamp=False, record, workspace):
    """struct rtxn_image_metrics_args over the given tensors (which the caller keeps alive): pred float32 with H*W*3 elements
    ([H*W, 3] as the compositor writes it, or [H, W, 3]), record float64 [3], workspace from image_metrics_workspace()."""
    n = image_set.width * image_set.height
    if pred.numel() != 3 * n or pred.shape[-1] != 3:
        raise _lib.RtxnError(f"image_metrics: pred of shape {tuple(pred.shape)}: [{n}, 3] or [{image_set.height}, {image_set.width}, 3]")
    if record.numel() != 3:
        raise _lib.RtxnError(f"image_metrics: record of shape {tuple(record.shape)}: [3]")
    if image_set.channels == 4 and background is None:
        raise _lib.RtxnError("image_metrics: a 4-channel image set needs background=(r, g, b) to composite its frames over")
    a = _lib.ImageMetricsArgs()
    a.set = image_set.c_struct()
    a.image = int(image)
    a.pred = _ptr(pred, torch.float32, "pred")
    if background is not None:
        bg = [float(v) for v in background]
        if len(bg) != 3:
            raise _lib.RtxnError(f"image_metrics: background {background!r}: three floats")
        a.background[:] = bg
    a.flags = (METRICS_SSIM if ssim else 0) | (METRICS_CLAMP if clamp else 0)
    a.workspace, a.workspace_bytes = _ptr(workspace, torch.uint8, "workspace"), workspace.numel()
    a.record = _ptr(record, torch.float64, "record")
    return a


def image_metrics(image_set, image, pred, *, background=None, ssim=True, clamp=False, record=None, workspace=None):
    """rtxn_image_metrics: (mse, psnr, ssim) of the rendered frame `pred` against frame `image` of image_set, as a float64 device
    tensor of 3 (`record`, or a new one), on the current stream with nothing read on the host.  background: three floats a
    4-channel set's frames are composited over (required for one, ignored for RGB); ssim=False leaves NaN in slot 2 and takes
    frames smaller than 11 x 11; clamp: pred is clamped to [0, 1] first, as an 8-bit PNG of it would be."""
    if record is None:
        record = torch.empty(3, dtype=torch.float64, device=pred.device)
    if workspace is None:
        workspace = image_metrics_workspace(image_set)
    a = image_metrics_args(image_set, image, pred, background=background, ssim=ssim, clamp=clamp, record=record, workspace=workspace)
    check(_lib.lib().rtxn_image_metrics(C.byref(a), _stream()), "rtxn_image_metrics")
    return record


# --------------------------------------------------------------------------- ray gradients and pose refinement
def ray_gradients(t_start, t_end, dstart, dend, d_origin, d_direction):
    """struct rtxn_ray_gradients (include/rtxn.h) over device float32 tensors (which the struct keeps referenced): t_start, t_end
    [>= segments] as trace_grid writes them (TRACE_DDA), dstart, dend [>= segments, 3], d_origin, d_direction [>= n_rays, 3]."""
    s = _lib.RayGradients()
    s._tensors = dict(t_start=t_start, t_end=t_end, dstart=dstart, dend=dend, d_origin=d_origin, d_direction=d_direction)
    for nm, t in s._tensors.items():
        setattr(s, nm, _ptr(t, torch.float32, nm))
    return s


def _check_ray_gradients(who, rays, n_rays, n_segments):
    tensors = getattr(rays, "_tensors", None)      # a _lib.RayGradients filled by hand: nothing to size, the library checks the rest
    if tensors is None:
        return
    for nm, need in (("t_start", n_segments), ("t_end", n_segments), ("dstart", 3 * n_segments), ("dend", 3 * n_segments),
                     ("d_origin", 3 * n_rays), ("d_direction", 3 * n_rays)):
        t = tensors[nm]
        if t is not None and t.numel() < int(need):
            raise _lib.RtxnError(f"{who}: rays.{nm} holds {t.numel()} elements, {int(need)} needed")


def ray_gradients_supported(net, grid=None):
    """rtxn_ray_gradients_supported: whether a step of this model forms d(encoding) -- hash-grid models do."""
    return bool(_lib.lib().rtxn_ray_gradients_supported(net._h if net is not None else None, grid._h if grid is not None else None))


def hashgrid_input_gradient_segments(grid, table_fp16, start_points, end_points, n_segments, sample_type, dencT, dstart, dend, *, live_ws=None,
                                     jitter=None, loss_scale=1.0, scale_device=None):
    """rtxn_hashgrid_input_gradient_segments: dstart, dend float32 [>= n_segments, 3] = k times the (1 - u)- and u-weighted sums of
    every segment's 32 sample gradients dL/dx, from dencT as the scatter takes it.  k = 1 / loss_scale (float32), or with
    scale_device (a device float32 tensor, the scaler's loss_scale_now) 1 / its value, read on the device.  live_ws: the listed
    segments only, every other segment of the batch reads back as zeros."""
    n = int(n_segments)
    for nm, t in (("dstart", dstart), ("dend", dend)):
        if t.numel() < 3 * n:
            raise _lib.RtxnError(f"hashgrid_input_gradient_segments: {nm} holds {t.numel()} elements, {3 * n} needed")
    if dencT.numel() < grid.cfg.n_levels * grid.cfg.n_features * padded_samples(32 * n):
        raise _lib.RtxnError(f"hashgrid_input_gradient_segments: dencT holds {dencT.numel()} elements for {n} segments")
    check(_lib.lib().rtxn_hashgrid_input_gradient_segments(
        grid._h, _ptr(table_fp16, torch.float16, "table"), _ptr(start_points, torch.float32, "start_points"),
        _ptr(end_points, torch.float32, "end_points"), n, sample_type, _ptr(dencT, torch.float16, "dencT"), _ptr(live_ws, None, "live_ws"),
        _jit(jitter), float(np.float32(1.0) / np.float32(loss_scale)), _ptr(scale_device, torch.float32, "scale_device"),
        _ptr(dstart, torch.float32, "dstart"), _ptr(dend, torch.float32, "dend"), _stream()), "rtxn_hashgrid_input_gradient_segments")
    return dstart, dend


def ray_gradients_reduce(indices, num_stored, t_start, t_end, dstart, dend, n_rays, d_origin, d_direction):
    """rtxn_ray_gradients_reduce: d_origin, d_direction float32 [>= n_rays, 3] from the segments' end-point gradients."""
    n = int(n_rays)
    for nm, t, need in (("indices", indices, n), ("num_stored", num_stored, n), ("d_origin", d_origin, 3 * n), ("d_direction", d_direction, 3 * n)):
        if t.numel() < need:
            raise _lib.RtxnError(f"ray_gradients_reduce: {nm} holds {t.numel()} elements, {need} needed")
    check(_lib.lib().rtxn_ray_gradients_reduce(_ptr(indices, torch.int32, "indices"), _ptr(num_stored, torch.int32, "num_stored"),
                                               _ptr(t_start, torch.float32, "t_start"), _ptr(t_end, torch.float32, "t_end"),
                                               _ptr(dstart, torch.float32, "dstart"), _ptr(dend, torch.float32, "dend"), n,
                                               _ptr(d_origin, torch.float32, "d_origin"), _ptr(d_direction, torch.float32, "d_direction"),
                                               _stream()), "rtxn_ray_gradients_reduce")
    return d_origin, d_direction


def pose_refinement(n_images=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15, *, poses0=None, poses=None, delta=None, m=None, v=None,
                    steps=None, grad=None, skip=None, skipped=None, drawn=None):
    """struct rtxn_pose_refinement (include/rtxn.h), its rules checked (rtxn_pose_refinement_check) before any buffer is looked at.
    Without tensors: the configuration alone (what a caller checks before it allocates).  poses0, poses float32 [n, 16]; delta, m,
    v float32 [n, 6]; steps int32 [n]; grad float32 [n, 8]; skip: the optimizer guard's skip word (guard[2:3]) or None; skipped:
    int32 [1] or None; drawn int32 [n_rays, 2] (train_step only).  The tensors stay referenced by the struct."""
    s = _lib.PoseRefinement()
    s.n_images, s.lr, s.beta1, s.beta2, s.eps = int(n_images), float(lr), float(beta1), float(beta2), float(eps)
    check(_lib.lib().rtxn_pose_refinement_check(C.byref(s)), "rtxn_pose_refinement_check")
    n = s.n_images
    s._tensors = dict(poses0=poses0, poses=poses, delta=delta, m=m, v=v, steps=steps, grad=grad, skip=skip, skipped=skipped, drawn=drawn)
    for nm, t, dt, need in (("poses0", poses0, torch.float32, 16 * n), ("poses", poses, torch.float32, 16 * n), ("delta", delta, torch.float32, 6 * n),
                            ("m", m, torch.float32, 6 * n), ("v", v, torch.float32, 6 * n), ("steps", steps, torch.int32, n),
                            ("grad", grad, torch.float32, 8 * n), ("skip", skip, torch.int32, 1), ("skipped", skipped, torch.int32, 1),
                            ("drawn", drawn, torch.int32, 0)):
        if t is not None and t.numel() < need:
            raise _lib.RtxnError(f"pose_refinement: {nm} holds {t.numel()} elements, {need} needed for {n} images")
        setattr(s, nm, _ptr(t, dt, nm))
    return s


def pose_gradients(drawn, rays_d, d_origin, d_direction, n_rays, pose):
    """rtxn_pose_gradients: pose.grad[i] = (sum rays_d x d_direction, sum d_origin / 10, ray count, 0) over the rays drawn from image i."""
    n = int(n_rays)
    for nm, t, need in (("drawn", drawn, 2 * n), ("rays_d", rays_d, 3 * n), ("d_origin", d_origin, 3 * n), ("d_direction", d_direction, 3 * n)):
        if t.numel() < need:
            raise _lib.RtxnError(f"pose_gradients: {nm} holds {t.numel()} elements, {need} needed")
    check(_lib.lib().rtxn_pose_gradients(_ptr(drawn, torch.int32, "drawn"), _ptr(rays_d, torch.float32, "rays_d"),
                                         _ptr(d_origin, torch.float32, "d_origin"), _ptr(d_direction, torch.float32, "d_direction"), n,
                                         C.byref(pose), _stream()), "rtxn_pose_gradients")


def pose_step(pose):
    """rtxn_pose_step: the per-image Adam on delta from pose.grad, then poses = (R(omega) R0 | t0 + tau)."""
    check(_lib.lib().rtxn_pose_step(C.byref(pose), _stream()), "rtxn_pose_step")


def pose_compose(pose):
    """rtxn_pose_compose: poses from delta and poses0 alone (after a checkpoint was loaded into delta, or a reset)."""
    check(_lib.lib().rtxn_pose_compose(C.byref(pose), _stream()), "rtxn_pose_compose")


# --------------------------------------------------------------------------- intrinsics refinement
CAMERA_DELTA = 10          # fx, fy, cx, cy, k1, k2, k3, k4, p1, p2
# Defaults of camera_refinement() / Trainer.attach_images(refine_cameras=True), chosen on the lens demo of DESIGN 5.21 (one seed):
# the distortion group is FROZEN by default -- the demo does not recover its coefficients -- and moves only with a rate of its own.
CAMERA_REFINE_DEFAULTS = dict(lr_focal=1e-3, lr_center=3e-2, lr_distortion=0.0, max_log_focal=0.25, max_center=8.0, max_distortion=0.05,
                              beta1=0.9, beta2=0.999, eps=1e-15)


def camera_refinement(model=CAMERA_PINHOLE, n_cameras=1, width=0, *, lr_focal=None, lr_center=None, lr_distortion=None, max_log_focal=None,
                      max_center=None, max_distortion=None, beta1=None, beta2=None, eps=None, params0=None, params=None, delta=None, m=None,
                      v=None, steps=None, grad=None, terms=None, skip=None, skipped=None, drawn=None, poses=None):
    """struct rtxn_camera_refinement (include/rtxn.h), its rules checked (rtxn_camera_refinement_check) before any buffer is looked
    at.  model: a CAMERA_* value or name; width: the frames' width.  A rate of 0 freezes its group (focal: fx, fy as
    fx0 exp(delta); centre: cx, cy in pixels; distortion: k1..k4, p1, p2); max_*: the clamp of the group's |delta|.  Without
    tensors: the configuration alone.  params0, params float32 [n, 12]; delta, m, v float32 [n, 10]; steps int32 [n]; grad float32
    [n, 12]; terms float32 [>= n_rays, 12] (the gradient's scratch); skip: the optimizer guard's skip word or None; skipped int32
    [1] or None; drawn int32 [n_rays, 2] and poses float32 [n_images, 16] (train_step only).  The tensors stay referenced."""
    s = _lib.CameraRefinement()
    s.model, s.n_cameras, s.width = int(CAMERA_MODELS.get(model, model)), int(n_cameras), int(width)
    cfg = dict(CAMERA_REFINE_DEFAULTS)
    cfg.update({k: val for k, val in dict(lr_focal=lr_focal, lr_center=lr_center, lr_distortion=lr_distortion, max_log_focal=max_log_focal,
                                          max_center=max_center, max_distortion=max_distortion, beta1=beta1, beta2=beta2, eps=eps).items()
                if val is not None})
    for k, val in cfg.items():
        setattr(s, k, float(val))
    check(_lib.lib().rtxn_camera_refinement_check(C.byref(s)), "rtxn_camera_refinement_check")
    n = s.n_cameras
    s._tensors = dict(params0=params0, params=params, delta=delta, m=m, v=v, steps=steps, grad=grad, terms=terms, skip=skip, skipped=skipped,
                      drawn=drawn, poses=poses)
    for nm, t, dt, need in (("params0", params0, torch.float32, CAMERA_PARAMS * n), ("params", params, torch.float32, CAMERA_PARAMS * n),
                            ("delta", delta, torch.float32, CAMERA_DELTA * n), ("m", m, torch.float32, CAMERA_DELTA * n),
                            ("v", v, torch.float32, CAMERA_DELTA * n), ("steps", steps, torch.int32, n), ("grad", grad, torch.float32, 12 * n),
                            ("terms", terms, torch.float32, 12), ("skip", skip, torch.int32, 1), ("skipped", skipped, torch.int32, 1),
                            ("drawn", drawn, torch.int32, 0), ("poses", poses, torch.float32, 16)):
        if t is not None and t.numel() < need:
            raise _lib.RtxnError(f"camera_refinement: {nm} holds {t.numel()} elements, {need} needed for {n} cameras")
        setattr(s, nm, _ptr(t, dt, nm))
    return s


def camera_gradients(drawn, d_direction, n_rays, set_poses, cameras):
    """rtxn_camera_gradients: cameras.grad[c] = (dL/d(fx, fy, cx, cy, k1..k4, p1, p2), ray count, 0) summed over the rays drawn
    with camera c (every ray for a shared camera), from dL/d(rays_d) and the poses the batch was drawn with."""
    n = int(n_rays)
    terms = getattr(cameras, "_tensors", {}).get("terms")
    for nm, t, need in (("drawn", drawn, 2 * n), ("d_direction", d_direction, 3 * n), ("terms", terms, 12 * n)):
        if t is not None and t.numel() < need:
            raise _lib.RtxnError(f"camera_gradients: {nm} holds {t.numel()} elements, {need} needed")
    check(_lib.lib().rtxn_camera_gradients(_ptr(drawn, torch.int32, "drawn"), _ptr(d_direction, torch.float32, "d_direction"), n,
                                           _ptr(set_poses, torch.float32, "set_poses"), C.byref(cameras), _stream()), "rtxn_camera_gradients")


def camera_step(cameras):
    """rtxn_camera_step: the per-camera three-group Adam on delta from cameras.grad, clamped, then the rows recomposed."""
    check(_lib.lib().rtxn_camera_step(C.byref(cameras), _stream()), "rtxn_camera_step")


def camera_compose(cameras):
    """rtxn_camera_compose: the rows from delta and params0 alone (after a checkpoint was loaded into delta, or a reset)."""
    check(_lib.lib().rtxn_camera_compose(C.byref(cameras), _stream()), "rtxn_camera_compose")
