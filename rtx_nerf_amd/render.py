"""The render hot path on one GPU, as a caller of librtxn's frame entry points (include/rtxn.h: rtxn_render_*).

Counterpart of the stage order of the reference's main loop (main.cu:463-543 traversal, :631-637 compaction, :704
sampler, :721 MLP, :728 glue, :737 compositing), minus its host round trips: the reference copies every traversal
buffer to the host, mallocs four arrays per ray, re-packs the batch on the CPU and cudaMalloc/cudaFrees six buffers per
batch.  Here the whole frame

    trace (count) -> scan -> trace (write packed CSR) -> sampler+encode+MLP (one kernel) -> volume render

is ONE C call (rtxn_render_frame; rtxn_render_frame_async for the three-stream pipelined form) that enqueues every stage
without a host synchronisation; a C++ host gets exactly the same frame (examples/render_host.cpp).  This module only owns
the workspace tensor, maps torch views onto the slot buffers for tests and tools, and applies the overflow policy.

Radiance model: an api.Network with the reference's Composite-Frequency encoding (fused frequency kernels), or -- with
hashgrid= / table= -- a pre-encoded 64-wide api.Network behind an api.HashGrid (the fused hash-encode + MLP kernel): what
train.Trainer(encoding="hash") trains.
"""
import ctypes as C

import torch

from . import _lib, api

RENDER_FLOAT4 = 1     # enum rtxn_render_flags
RENDER_STABLE_INPUTS = 2
RENDER_AUX = 4        # the traversal also keeps each segment's entry / exit distance: the depth output of render_ex


class RenderPipeline:
    def __init__(self, network, grid_res, width, height, focal_length, aspect_ratio=None, occupancy=None,
                 max_rays=None, max_segments=None, trace_mode=api.TRACE_DDA, vr_mode=api.VR_COMPAT,
                 device="cuda", window=(0, 0), step_scale=1.0, sub_rays=None, compact=None, on_overflow="raise",
                 hashgrid=None, table=None, sample_type=None, n_slots=None, stable_inputs=False, aux=False,
                 min_transmittance=None, first_round_segments=4, termination_rounds=5, per_ray=True):
        self.net = network
        self.hg, self.table = hashgrid, table
        if (hashgrid is None) != (table is None):
            raise ValueError("hashgrid= and table= go together")
        self.R = grid_res
        self.W, self.H = width, height
        self.focal = float(focal_length)
        self.aspect = float(width) / float(height) if aspect_ratio is None else float(aspect_ratio)
        self.trace_mode, self.vr_mode = trace_mode, vr_mode
        self.window = window   # (chunk, stride) ray interleave of this shard, see rtxn_trace_params
        # sub_rays = Q in {2,4,8,16,..}: Q lanes walk consecutive pieces of each ray (rtxn_trace_params.sub_rays): same
        # segments bit for bit, a shorter critical path -- worth it when the launch is small (a shard, a training batch)
        n_rays = width * height if max_rays is None else max_rays
        self.sub_rays = (api.auto_sub_rays(n_rays) if sub_rays is None else int(sub_rays)) if trace_mode == api.TRACE_DDA else 0
        self.step_scale = float(step_scale)
        # sample placement: the frequency model's fused kernel samples REGULAR (sampler.cu:52-66); a hash model defaults to
        # what its compositor wants (RTXN_VR_NERF: sub-interval midpoints + world-space steps, as train.Trainer's "nerf" mode)
        if sample_type is None:
            sample_type = api.SAMPLING_MIDPOINT_WORLD if (hashgrid is not None and vr_mode == api.VR_NERF) else api.SAMPLING_REGULAR
        self.sample_type = sample_type
        # compact (default wherever it applies): the MLP kernel hands the compositor the network's own half outputs
        # (8 B/sample) and no per-sample t_vals -- bit-identical pixels at 40 % of the intermediate's bytes (0.8 instead of
        # 2.0 GB per bench frame).  compact=False: the reference's convertHalfToFloat layout (float4 + t_vals), frequency model.
        if compact is None:
            compact = hashgrid is not None or vr_mode == api.VR_COMPAT
        self.compact = bool(compact)
        if self.compact and hashgrid is None and vr_mode != api.VR_COMPAT:
            raise ValueError("the frequency model's compact hand-over is RTXN_VR_COMPAT only (REGULAR t_vals are implicit)")
        self.dev = torch.device(device)
        # A pose that needs more segments than the buffers hold is cut off ON THE DEVICE (never out of bounds).  So that
        # this cannot pass unnoticed outside the calibrated pose set, every frame copies its segment count to pinned host
        # memory (4 bytes, async, inside rtxn_render_frame) and the NEXT call -- or finish() -- looks at the counts that have
        # arrived (rtxn_render_status): on_overflow = "raise" (default): RuntimeError; "grow": re-create the renderer at 1.5x
        # the need (a pipeline stall, once) and go on -- the cut frame was delivered truncated either way and is counted in
        # overflow_frames; "ignore": count only.
        if on_overflow not in ("raise", "grow", "ignore"):
            raise ValueError("on_overflow must be 'raise', 'grow' or 'ignore'")
        self.on_overflow = on_overflow
        # stable_inputs: the caller's promise for render_async (RTXN_RENDER_STABLE_INPUTS, include/rtxn.h): device poses are
        # uploaded before the call and left alone until their frame has been traversed.  Without it the traversal of every
        # pipelined frame waits for the caller's stream (correct for a pose buffer rewritten per frame, ~3 % slower).
        self.stable_inputs = bool(stable_inputs)
        self.overflow_frames = 0
        self.occ = occupancy
        self.max_rays = n_rays
        # default capacity: every ray crossing a full grid diagonal's worth of occupied cells is far too
        # pessimistic; callers size it from a counting pass (see calibrate())
        self.max_segments = int(max_segments) if max_segments is not None else 16 * n_rays
        import os
        self.n_slots = int(n_slots) if n_slots else int(os.environ.get("RTXN_ASYNC_SLOTS", "3"))
        self.pixels = torch.empty((n_rays, 3), device=self.dev)
        # aux: depth output of render_ex (RTXN_RENDER_AUX: +8 B per segment of capacity and slot); opacity and the background
        # work on every pipeline
        self.aux = bool(aux)
        self.depth = torch.empty(n_rays, device=self.dev) if self.aux else None
        self.opacity = torch.empty(n_rays, device=self.dev)
        self.look_at = torch.zeros(16, device=self.dev)
        # early termination (rtxn_render_set_termination): render / render_ex / capture[_ex] shade each ray front to back in
        # `termination_rounds` rounds (first_round_segments * 2^k segments per living ray, the last round the rest) and stop a
        # ray once exp(-optical depth) < min_transmittance at a round boundary: every output moves by at most
        # min_transmittance (depth: times the largest sample distance).  None = off: the plain frame.
        self.min_transmittance = None if min_transmittance is None else float(min_transmittance)
        self.first_round_segments, self.termination_rounds = int(first_round_segments), int(termination_rounds)
        # per_ray=False: keep the per-segment direction product (the seg_view entries) where the model has per-ray kernels too
        self.per_ray = bool(per_ray)
        self._term_ws = None
        self._ray_ws = None
        self._cam_rays = None      # render_camera(): the frame's explicit rays, float32 [W*H, 3] x 2, made on first use
        self._h = None
        self._comp_stream = None
        self._create()

    # ------------------------------------------------------------------------------------------ the C renderer
    def _config(self):
        c = _lib.RenderConfig()
        c.mlp = self.net._h
        c.grid = self.hg._h if self.hg is not None else None
        c.table_fp16 = api._ptr(self.table, torch.float16, "table") if self.table is not None else None
        c.n_dir_freqs = self.hg.n_dir_freqs if self.hg is not None else 0
        c.width, c.height = self.W, self.H
        c.focal_length, c.aspect_ratio = self.focal, self.aspect
        c.max_rays = self.max_rays
        c.window_chunk, c.window_stride = self.window
        c.grid_res = self.R
        c.occupancy = api._ptr(self.occ, torch.int32, "occupancy") if self.occ is not None else None
        c.trace_mode, c.sub_rays = self.trace_mode, self.sub_rays
        c.vr_mode, c.sample_type, c.step_scale = self.vr_mode, self.sample_type, self.step_scale
        c.max_segments = self.max_segments
        c.n_slots = self.n_slots
        c.flags = ((0 if self.compact else RENDER_FLOAT4) | (RENDER_STABLE_INPUTS if self.stable_inputs else 0)
                   | (RENDER_AUX if self.aux else 0))
        return c

    def _destroy(self):
        h, self._h = self._h, None
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:
            _lib._lib.rtxn_render_destroy(h)

    def __del__(self):
        self._destroy()

    def _create(self):
        """(Re)create the C renderer for the current max_segments: one workspace tensor, laid out by librtxn."""
        self._destroy()
        lib = _lib.lib()
        cfg = self._config()
        need = lib.rtxn_render_workspace_bytes(C.byref(cfg))
        if need == 0:
            msg = lib.rtxn_last_error()
            raise _lib.RtxnError(f"rtxn_render_workspace_bytes: {msg.decode() if msg else '?'}")
        self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        h = C.c_void_p()
        _lib.check(lib.rtxn_render_create(C.byref(cfg), C.c_void_p(self._ws.data_ptr()), need, C.byref(h)), "rtxn_render_create")
        self._h = h
        self._seen_overflows = 0
        # per-ray shading (rtxn_render_set_ray_workspace): wherever the model has the kernels, in a second tensor of the same
        # lifetime -- each segment's ray and, per slot, the table of layer 0's direction product over the rays
        self._ray_ws = None
        ray_need = lib.rtxn_render_ray_workspace_bytes(C.byref(cfg)) if self.per_ray else 0
        if ray_need:
            self._ray_ws = torch.empty(ray_need, dtype=torch.uint8, device=self.dev)
            _lib.check(lib.rtxn_render_set_ray_workspace(h, C.c_void_p(self._ray_ws.data_ptr()), ray_need), "rtxn_render_set_ray_workspace")
        self._slots = [self._slot_views(i) for i in range(self.n_slots)]
        for f in ("num_hits", "num_hits_c", "indices", "total", "start", "end", "seg_view", "radiance", "t_vals", "seg_step", "view_dirs", "seg_ray",
                  "ray_bias"):
            setattr(self, f, getattr(self._slots[0], f))
        self._term_ws = None
        if self.min_transmittance is not None:
            self.set_termination(self.min_transmittance, self.first_round_segments, self.termination_rounds)

    # ------------------------------------------------------------------------------------------ early termination
    def set_termination(self, min_transmittance=None, first_round_segments=4, termination_rounds=5):
        """Set (or, with min_transmittance=None, clear) early termination on the C renderer.  Setting it allocates the
        second workspace (one round's packed scratch per slot + per-ray state), synchronises the device and resets
        termination_stats(); render_async* raise while it is set."""
        lib = _lib.lib()
        if min_transmittance is None:
            _lib.check(lib.rtxn_render_set_termination(self._h, None, None, 0), "rtxn_render_set_termination")
            self.min_transmittance = None
            return
        t = _lib.RenderTermination(float(min_transmittance), int(first_round_segments), int(termination_rounds))
        cfg = self._config()
        need = lib.rtxn_render_termination_workspace_bytes(C.byref(cfg), C.byref(t))
        if need == 0:
            msg = lib.rtxn_last_error()
            raise _lib.RtxnError(f"rtxn_render_termination_workspace_bytes: {msg.decode() if msg else '?'}")
        ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        _lib.check(lib.rtxn_render_set_termination(self._h, C.byref(t), C.c_void_p(ws.data_ptr()), need), "rtxn_render_set_termination")
        self._term_ws = ws                     # the previous one (if any) is released only now: the setter has synchronised
        self.min_transmittance = float(min_transmittance)
        self.first_round_segments, self.termination_rounds = int(first_round_segments), int(termination_rounds)

    def termination_stats(self, wait=True):
        """struct rtxn_render_termination_stats as a dict (wait: synchronise first, so every enqueued or replayed frame counts)."""
        st = _lib.RenderTerminationStats()
        _lib.check(_lib.lib().rtxn_render_termination_status(self._h, 1 if wait else 0, C.byref(st)), "rtxn_render_termination_status")
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def shaded_per_ray(self, slot=0):
        """int32[max_rays] view of the segments of each ray the slot's last terminated frame shaded (device; no copy)."""
        if self._term_ws is None:
            raise RuntimeError("shaded_per_ray: early termination has not been set on this pipeline")
        p = C.c_void_p()
        _lib.check(_lib.lib().rtxn_render_termination_buffers(self._h, slot, C.byref(p)), "rtxn_render_termination_buffers")
        off = p.value - self._term_ws.data_ptr()
        return self._term_ws[off:off + 4 * self.max_rays].view(torch.int32)

    def _slot_views(self, i):
        """torch views of slot i's device buffers inside the workspace (tests, tools; the C side owns the layout)."""
        from types import SimpleNamespace
        ptrs = [C.c_void_p() for _ in range(11)]
        _lib.check(_lib.lib().rtxn_render_slot_buffers(self._h, i, *[C.byref(p) for p in ptrs]), "rtxn_render_slot_buffers")
        base, n, m, K = self._ws.data_ptr(), self.max_rays, self.max_segments, api.NUM_SAMPLES_PER_SEGMENT

        def view(p, count, dtype, shape, ws=None, origin=None):
            off = p.value - (base if origin is None else origin)
            nbytes = count * torch.empty((), dtype=dtype).element_size()
            return (self._ws if ws is None else ws)[off:off + nbytes].view(dtype).view(shape)

        g = SimpleNamespace()
        g.num_hits = view(ptrs[0], n, torch.int32, (n,))
        g.num_hits_c = view(ptrs[1], n, torch.int32, (n,))      # segments actually stored per ray
        g.indices = view(ptrs[2], n, torch.int32, (n,))
        g.total = view(ptrs[3], 1, torch.int32, (1,))
        g.start = view(ptrs[4], 3 * m, torch.float32, (m, 3))
        g.end = view(ptrs[5], 3 * m, torch.float32, (m, 3))
        g.seg_view = view(ptrs[6], 2 * m, torch.float32, (m, 2))
        g.radiance = (view(ptrs[7], m * K * 4, torch.float16, (m * K, 4)) if self.compact
                      else view(ptrs[7], m * K * 4, torch.float32, (m * K, 4)))
        g.t_vals = view(ptrs[8], m * K, torch.float32, (m * K,)) if ptrs[8].value else None
        g.seg_step = view(ptrs[9], m, torch.float32, (m,)) if ptrs[9].value else None
        g.view_dirs = view(ptrs[10], 2 * n, torch.float32, (n, 2))
        # per-ray shading (rtxn_mlp_forward_segments_rays): each segment's ray and the rays' table of layer 0's direction
        # product, in the ray workspace; None where the frame shades through seg_view
        rp = [C.c_void_p(), C.c_void_p()]
        _lib.check(_lib.lib().rtxn_render_ray_buffers(self._h, i, C.byref(rp[0]), C.byref(rp[1])), "rtxn_render_ray_buffers")
        g.seg_ray = g.ray_bias = None
        if rp[0].value:
            Wn, rbase = self.net.cfg.n_neurons, self._ray_ws.data_ptr()
            g.seg_ray = view(rp[0], m, torch.int32, (m,), self._ray_ws, rbase)
            g.ray_bias = view(rp[1], n * Wn, torch.float32, (n, Wn), self._ray_ws, rbase)
        return g

    def _status(self, wait=False):
        st = _lib.RenderStats()
        _lib.check(_lib.lib().rtxn_render_status(self._h, 1 if wait else 0, C.byref(st)), "rtxn_render_status")
        return st

    def _check_overflow(self, wait=False):
        """Apply the overflow policy to the frames whose segment count has reached the host (no synchronisation unless
        `wait`: the caller then wants every enqueued frame looked at)."""
        if torch.cuda.is_current_stream_capturing():
            return
        st = self._status(wait)
        new = st.overflow_frames - self._seen_overflows
        if new <= 0:
            return
        self._seen_overflows = st.overflow_frames
        self.overflow_frames += new
        need = int(st.max_segments_needed)
        if self.on_overflow == "raise":
            raise RuntimeError(f"RenderPipeline: a frame needed {need} segments but the buffers hold {self.max_segments}: its rays "
                               f"were truncated.  calibrate() with that pose, raise max_segments, or use on_overflow='grow'")
        if self.on_overflow == "grow":
            torch.cuda.synchronize()                      # frames in flight still use the old buffers
            self.max_segments = int(need * 1.5) + 1024
            self._create()

    # ------------------------------------------------------------------------------------------ frames
    def set_pose(self, look_at):
        """look_at: 16 floats (host or device), row-major camera-to-world (params.h:17)."""
        self.look_at.copy_(torch.as_tensor(look_at, dtype=torch.float32).reshape(16), non_blocking=True)

    def set_occupancy(self, occupancy):
        """Point the renderer at an updated occupancy bitfield of the same resolution (rebuilds the mip / brick hierarchy)."""
        self.occ = occupancy
        _lib.check(_lib.lib().rtxn_render_set_occupancy(self._h, api._ptr(occupancy, torch.int32, "occupancy"), api._stream()),
                   "rtxn_render_set_occupancy")

    def count_segments(self, ray_begin=0, ray_count=None):
        """Counting pass + scan for the current pose; returns the number of segments (host int, synchronises)."""
        n = self.max_rays if ray_count is None else ray_count
        out = C.c_long(0)
        _lib.check(_lib.lib().rtxn_render_count_segments(self._h, C.c_void_p(self.look_at.data_ptr()), ray_begin, n, C.byref(out),
                                                         api._stream()), "rtxn_render_count_segments")
        return int(out.value)

    def count_segments_rays(self, rays_o, rays_d, ray_begin=0, ray_count=None):
        """count_segments() over explicit rays (rtxn_render_count_segments_rays); rays as render_rays() takes them."""
        n = self.max_rays if ray_count is None else ray_count
        out = C.c_long(0)
        _lib.check(_lib.lib().rtxn_render_count_segments_rays(self._h, *self._rays(rays_o, rays_d), ray_begin, n, C.byref(out),
                                                              api._stream()), "rtxn_render_count_segments_rays")
        return int(out.value)

    def calibrate(self, poses, ray_begin=0, ray_count=None, margin=1.10, cameras=None):
        """Size the segment buffers for a set of poses (outside any timed region).  cameras: an api.CameraSet of one camera or
        one per pose: pose i is counted over the rays of its camera (rtxn_render_count_segments_rays)."""
        worst = 0
        for i, p in enumerate(poses):
            self.set_pose(p)
            if cameras is not None:
                rays = self._camera_rays(cameras, 0 if cameras.n_cameras == 1 else i, None)
                worst = max(worst, self.count_segments_rays(*rays, ray_begin, ray_count))
                continue
            worst = max(worst, self.count_segments(ray_begin, ray_count))
        need = int(worst * margin) + 1024
        if need > self.max_segments or need < self.max_segments // 2:
            torch.cuda.synchronize()
            self.max_segments = need
            self._create()
        return worst

    def _pose(self, look_at):
        """the frame's pose: the one set_pose() wrote, or `look_at`, 16 device floats read where they lie (a row of an
        api.ImageSet's poses, say)"""
        if look_at is None:
            return C.c_void_p(self.look_at.data_ptr())
        if look_at.numel() != 16:
            raise ValueError(f"look_at of shape {tuple(look_at.shape)}: 16 floats")
        return api._ptr(look_at, torch.float32, "look_at")

    def render(self, ray_begin=0, ray_count=None, out=None, look_at=None):
        """Enqueue one frame (or one shard of it) on the current stream; returns the
        pixel buffer view float[ray_count, 3] (or `out`).  No host synchronisation.  look_at: see _pose()."""
        n = self.max_rays if ray_count is None else ray_count
        pixels = self.pixels[:n] if out is None else out
        self._check_overflow()
        _lib.check(_lib.lib().rtxn_render_frame(self._h, 0, self._pose(look_at), ray_begin, n,
                                                api._ptr(pixels, torch.float32, "pixels"), api._stream()), "rtxn_render_frame")
        return pixels

    def _outputs(self, n, background, depth, opacity, out):
        """struct rtxn_render_outputs over the pipeline's buffers (or out = (pixels, depth, opacity))."""
        if out is None:
            out = (self.pixels[:n], self.depth[:n] if self.depth is not None else None, self.opacity[:n])
        pixels, d, a = out
        if depth and d is None:
            raise ValueError("render_ex(depth=True) needs a pipeline built with aux=True (RTXN_RENDER_AUX)")
        o = _lib.RenderOutputs()
        o.pixels = api._ptr(pixels, torch.float32, "pixels")
        o.depth = api._ptr(d, torch.float32, "depth") if depth else None
        o.opacity = api._ptr(a, torch.float32, "opacity") if opacity else None
        if background is not None:
            o.background[:] = [float(v) for v in background]
        return o, (pixels, d if depth else None, a if opacity else None)

    def render_ex(self, ray_begin=0, ray_count=None, background=None, depth=True, opacity=True, out=None, look_at=None):
        """render() with the expected depth (sum w_i d_i, unnormalised; float[ray_count]) and the opacity (sum w_i) of every
        ray, and an optional background colour (3 floats) composited as (1 - opacity) * background (rtxn_render_frame_ex).
        Returns (pixels, depth, opacity); an output not asked for is None.  With no background the pixels are render()'s
        bit for bit.  look_at: see _pose()."""
        n = self.max_rays if ray_count is None else ray_count
        o, res = self._outputs(n, background, depth, opacity, out)
        self._check_overflow()
        _lib.check(_lib.lib().rtxn_render_frame_ex(self._h, 0, self._pose(look_at), ray_begin, n, C.byref(o),
                                                   api._stream()), "rtxn_render_frame_ex")
        return res

    def _rays(self, rays_o, rays_d):
        n = self.W * self.H
        for t, nm in ((rays_o, "rays_o"), (rays_d, "rays_d")):
            if t.numel() != 3 * n or t.shape[-1] != 3:
                raise ValueError(f"{nm} of shape {tuple(t.shape)}: [{n}, 3], one ray per pixel of the {self.W} x {self.H} launch")
        return api._ptr(rays_o, torch.float32, "rays_o"), api._ptr(rays_d, torch.float32, "rays_d")

    def render_rays(self, rays_o, rays_d, ray_begin=0, ray_count=None, background=None, depth=False, opacity=False, out=None):
        """render_ex() over the CALLER'S rays (rtxn_render_frame_rays): rays_o, rays_d float32 [W*H, 3] on the device, indexed by
        launch ray (what api.camera_rays writes), rays_d unit vectors; the pipeline's focal length and pose are not read.  The
        window and the configured interleave select rays as they do for a pose.  Returns (pixels, depth, opacity), an output
        not asked for None; with nothing but pixels asked for, the plain compositor runs.  The rays must stay untouched until
        the frame has run.  Capturable."""
        n = self.max_rays if ray_count is None else ray_count
        o, res = self._outputs(n, background, depth, opacity, out)
        self._check_overflow()
        _lib.check(_lib.lib().rtxn_render_frame_rays(self._h, 0, *self._rays(rays_o, rays_d), ray_begin, n, C.byref(o), api._stream()),
                   "rtxn_render_frame_rays")
        return res

    def _camera_rays(self, cameras, camera, look_at, ray_begin=0, ray_count=None):
        """enqueue: the frame's rays under `cameras[camera]` and the pose (_pose()) into the pipeline's own buffers"""
        if self._cam_rays is None:
            self._cam_rays = (torch.empty((self.W * self.H, 3), device=self.dev), torch.empty((self.W * self.H, 3), device=self.dev))
        pose = self.look_at if look_at is None else look_at
        if ray_count is None or self.window[0]:          # an interleaved window reaches past [ray_begin, ray_begin + ray_count)
            ray_begin, ray_count = 0, None
        return api.camera_rays(cameras, camera, pose, self.W, self.H, ray_begin, ray_count, *self._cam_rays)

    def render_camera(self, cameras, camera, look_at=None, ray_begin=0, ray_count=None, background=None, depth=False, opacity=False,
                      out=None):
        """One frame of camera `camera` of an api.CameraSet under look_at (16 device floats; None: set_pose()'s): rtxn_camera_rays
        into two [W*H, 3] buffers the pipeline owns (allocated on the first call -- make that one outside a graph capture), then
        render_rays() over them.  Two launches more than a pose frame, nothing on the host; capturable.  One frame at a time per
        pipeline: the next call rewrites the rays."""
        rays = self._camera_rays(cameras, camera, look_at, ray_begin, ray_count)
        return self.render_rays(*rays, ray_begin, ray_count, background, depth, opacity, out)

    def finish(self):
        """Wait for every enqueued frame and apply the overflow policy to all of them (raises under "raise")."""
        self.drain_async()
        torch.cuda.synchronize()
        self._check_overflow(wait=True)

    # A frame is three dependent stages with very different bounds: traversal (two latency-bound passes + scan, ~0.45 ms
    # whatever the ray count), the MLP kernel (MFMA-bound, 96 % of the time) and the compositor (HBM-bound).
    # rtxn_render_frame_async puts them on three HIP streams and rotates through n_slots buffer slots, so that while the MLP
    # kernel of frame i runs, frame i+1 is traversed and frame i-1 composited (DESIGN.md 5.1 has the measurements).  The host
    # never synchronises; it simply runs ahead.  This matters most when the frame is sharded over N GPUs (the fixed
    # traversal latency is 16 % of a rank's frame at N = 8).
    def render_async(self, look_at, ray_begin=0, ray_count=None, out=None):
        """Enqueue one frame, software-pipelined against its neighbours.  look_at: 16 floats -- a DEVICE tensor (copied into
        the slot on the traversal stream, which waits for the current stream first unless the pipeline was built with
        stable_inputs=True) or a HOST array / CPU tensor (rtxn_render_frame_async_host: staged through pinned memory, fully
        overlapped).  Returns (pixels, None, comp_stream): `pixels` is complete on `comp_stream`; follow-up work on it (a
        gather, a copy) is best enqueued there, or call drain_async()."""
        n = self.max_rays if ray_count is None else ray_count
        pixels = self.pixels[:n] if out is None else out
        self._check_overflow()
        comp = C.c_void_p()
        if isinstance(look_at, torch.Tensor) and look_at.is_cuda:
            _lib.check(_lib.lib().rtxn_render_frame_async(self._h, api._ptr(look_at, torch.float32, "look_at"), ray_begin, n,
                                                          api._ptr(pixels, torch.float32, "pixels"), api._stream(), C.byref(comp)),
                       "rtxn_render_frame_async")
        else:
            import numpy as np
            host = np.ascontiguousarray(np.asarray(look_at, dtype=np.float32).reshape(16))
            _lib.check(_lib.lib().rtxn_render_frame_async_host(self._h, host.ctypes.data_as(C.POINTER(C.c_float)), ray_begin, n,
                                                               api._ptr(pixels, torch.float32, "pixels"), api._stream(), C.byref(comp)),
                       "rtxn_render_frame_async_host")
        if self._comp_stream is None or self._comp_stream.cuda_stream != comp.value:
            self._comp_stream = torch.cuda.ExternalStream(comp.value, device=self.dev)
        return pixels, None, self._comp_stream

    def render_async_ex(self, look_at, ray_begin=0, ray_count=None, background=None, depth=True, opacity=True, out=None):
        """render_async() with render_ex()'s outputs (rtxn_render_frame_async_ex).  Returns (pixels, depth, opacity,
        comp_stream): all three are complete on `comp_stream`."""
        n = self.max_rays if ray_count is None else ray_count
        o, res = self._outputs(n, background, depth, opacity, out)
        self._check_overflow()
        comp = C.c_void_p()
        if isinstance(look_at, torch.Tensor) and look_at.is_cuda:
            la, on_host = api._ptr(look_at, torch.float32, "look_at"), 0
        else:
            import numpy as np
            host = np.ascontiguousarray(np.asarray(look_at, dtype=np.float32).reshape(16))
            la, on_host = C.c_void_p(host.ctypes.data), 1
        _lib.check(_lib.lib().rtxn_render_frame_async_ex(self._h, la, on_host, ray_begin, n, C.byref(o), api._stream(), C.byref(comp)),
                   "rtxn_render_frame_async_ex")
        if self._comp_stream is None or self._comp_stream.cuda_stream != comp.value:
            self._comp_stream = torch.cuda.ExternalStream(comp.value, device=self.dev)
        return res + (self._comp_stream,)

    def drain_async(self):
        """Make the current stream wait for every frame enqueued with render_async."""
        if self._h:
            _lib.check(_lib.lib().rtxn_render_drain(self._h, api._stream()), "rtxn_render_drain")

    def capture(self, ray_begin=0, ray_count=None, out=None):
        """Capture one frame into a hipGraph (torch.cuda.CUDAGraph over rtxn_render_frame: nothing in it allocates,
        synchronises or touches the host).  Returns (graph, pixels): update the pose with set_pose() and call graph.replay().
        The frame must have been rendered once eagerly (kernel attributes)."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pixels = self.render(ray_begin, ray_count, out)
        return g, pixels

    def capture_ex(self, ray_begin=0, ray_count=None, background=None, depth=True, opacity=True, out=None):
        """capture() over render_ex().  Returns (graph, pixels, depth, opacity).  The background is a kernel argument of the
        captured compositor: the graph keeps the background it was captured with."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            res = self.render_ex(ray_begin, ray_count, background, depth, opacity, out)
        return (g,) + res

    def overflowed(self):
        """True if a frame was ever truncated (synchronises: also looks at the frames still in flight)."""
        if self.on_overflow == "raise":
            st = self._status(wait=True)
            return self.overflow_frames > 0 or st.overflow_frames > 0
        self._check_overflow(wait=True)
        return self.overflow_frames > 0

    # ------------------------------------------------------------------------------------------ diagnostics
    def shade_again(self, slot=0):
        """Re-issue the sampler+encode+MLP launch of a frame over slot `slot`'s current segments, on the current stream -- the
        very launch rtxn_render_frame makes (same entry point, same buffers) -- so that tools can bracket the dominant kernel
        alone with HIP events (bench.py's roofline)."""
        g = self._slots[slot]
        if self.hg is not None:
            api.hashmlp_forward_segments(self.net, self.hg, self.table, g.start, g.end, g.seg_view, g.total, self.max_segments,
                                         g.radiance, self.sample_type, self.step_scale, g.seg_step)
        elif self.compact and g.ray_bias is not None:
            self.net.forward_segments_rays(g.start, g.end, g.seg_ray, g.ray_bias, g.total, self.max_segments, g.radiance)
        elif self.compact:
            self.net.forward_segments_compact(g.start, g.end, g.seg_view, g.total, self.max_segments, g.radiance)
        else:
            raise RuntimeError("shade_again: compact pipelines only")
