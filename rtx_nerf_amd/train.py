"""Training-step orchestration on one GPU: the counterpart of the reference's
training loop (main.cu:612-805) over the C ABI.

Per step (stage order of main.cu, host round trips removed):
  rays -> trace(count) -> scan -> trace(write packed CSR)        main.cu:463-543,631-673
       -> sampler                                                :704
       -> encoding + network->forward (activations kept)         :715-728
       -> volume render forward                                  :737
       -> L2 loss                                                :759
       -> volume render backward                                 :767
       -> network->backward (+ hash-grid scatter)                :781
       -> Adam on the fp32 master copy, fp16 params re-packed    :787
The reference's per-batch cudaMalloc/cudaFree (:667-694,794-801) and host re-pack
(:646-673) do not exist here: every buffer is allocated once at capacity.

`mode`: "compat" reproduces the reference's arithmetic (REGULAR samples,
RTXN_VR_COMPAT forward/backward -- whose backward is not the gradient of its
forward); "nerf" is the corrected path (midpoint samples, world-space
steps, exact gradients) that actually converges.  All arithmetic is in librtxn.so;
torch only owns buffers and a few trivial elementwise glue ops.
"""
import json
import os
import struct
import weakref

import numpy as np
import torch
import torch.distributed as dist

from . import api


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class _Stage:
    """HIP-event bracket around one stage of Trainer.step on the current stream (Trainer.time_stages)."""

    def __init__(self, tr, name):
        self.tr, self.name = tr, name

    def __enter__(self):
        if self.tr._stage_ev is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if self.tr._stage_ev is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.tr._stage_ev.append((self.name, self.e0, e1))
        return False


class Trainer:
    def __init__(self, grid_res, occupancy=None, encoding="hash", n_neurons=64, n_hidden_layers=4,
                 hashgrid=None, n_dir_freqs=4, batch_rays=4096, max_segments=None, lr=1e-3, loss_scale=128.0,
                 density_scale=1.0, mode="nerf", seed=1337, device="cuda", deterministic=None, background=None, background_seed=0,
                 target_channels=None, sample_jitter=False, jitter_seed=0, loss="l2", loss_param=None, opacity_weight=0.0,
                 distortion_weight=0.0, lr_schedule=None, weight_decay=0.0, skip_nonfinite=False, max_grad_norm=None,
                 ema_decay=None, ray_gradients=False, depth_weight=0.0, depth_loss="l2", depth_loss_param=None):
        """depth_weight: lambda_z of the depth term (librtxn: rtxn_train_depth, rtxn_volrender_depth_train /
        rtxn_train_gradients_depth / rtxn_train_step_depth): (lambda_z / n_rays) sum_r l(D_r - z_r) over the rays with a depth target
        z_r > 0, D_r = sum w m the ray's expected depth (not divided by its opacity), distances in world units along the ray; mode
        "nerf" and the fused compositor only.  depth_loss: "l2" | "l1" | "huber" (depth_loss_param: delta, default 0.1).  The
        targets come from the attached image set's depth maps (attach_images() then needs api.ImageSet(depth=...); the target
        kernel runs right behind every draw) or from the caller: step(..., depth_targets=) / gradients(..., depth_targets=), and
        graph_depth_targets beside graph_targets for the captured and one-call steps.  Trainer.depth holds D_r and
        Trainer.depth_loss l(e_r) of every ray of the last batch.  Like distortion_weight its gradient rides the fp16 radiance
        gradients.  The term has no state: checkpoints do not change.  0.0: nothing is allocated and every call is the one made
        without the argument.
        ray_gradients: leave dL/d(rays_o) and dL/d(rays_d) of every step's loss, unscaled, in rays_o_grad / rays_d_grad
        [batch_rays, 3] (the first n rows, after gradients(), step(), step_captured() and step_entry(); librtxn:
        rtxn_hashgrid_input_gradient_segments, rtxn_ray_gradients_reduce, rtxn_train_gradients_rays, rtxn_train_step_rays): the
        gather over d(encoding) behind the table scatter, then the per-ray reduction with the segment distances held fixed
        (instant-ngp's approximation).  Hash encoding only.  attach_images(refine_poses=...) builds the per-image pose correction on
        it.  False: nothing is allocated and every call is the one made without the argument.
        ema_decay: None, or a float d strictly inside (0, 1): keep the debiased exponential moving average of the weights
        (tiny-cuda-nn's EMA optimizer; librtxn: rtxn_weight_ema, rtxn_train_step_ema), s = d s + (1 - d) w after every
        APPLIED update -- inside the Adam kernels of step(), step_captured() and step_entry(), which share the one state and may be
        mixed.  The MLP's average is kept densely; the hash table's lazily under the sparse rule (only the entries Adam touches are
        brought up to date, the read-out catches the rest up), densely under RTXN_TABLE_ADAM=dense.  A step the non-finite guard
        skips does not move the average; the EMA does not switch the guard on, but its steps take their rate from the device rate
        kernel, as every step under lr_schedule / weight_decay / skip_nonfinite does.  ema_updates is a device tensor no stepping
        method reads; ema_parameters() reads the average out, sync_ema() refreshes the model render_pipeline(weights="ema") draws;
        checkpoints hold the accumulators, the stamps and the state.  None: nothing is allocated and every call is the one made
        without the argument.
        loss_scale: a float (fixed, the reference's), "dynamic" (api.loss_scaler()'s defaults: from 128, x2 per 2000 clean steps, x0.5
        per skipped step, within [1, 65536]), or api.loss_scaler(init_scale=..., growth_interval=..., ...) / a dict
        of its arguments: the scale lives in device memory, is multiplied by `backoff` when a step's gradients are not finite (the
        step is skipped) and by `growth` after growth_interval clean steps, and the compositor, the optimizer, the captured and the
        one-call step all read it there (librtxn: rtxn_loss_scaler, rtxn_train_step_scaled).  max_grad_norm: clip the
        total gradient norm (MLP and table together, unscaled) to this value by torch.nn.utils.clip_grad_norm_'s rule; with a float
        loss_scale the scale stays fixed (a power of two then) and only the clipping is added, through the same path.  Either one
        switches the non-finite guard on (skipped_steps), needs mode "nerf" and the fused compositor.  loss_scale_now, grad_norm,
        clipped_steps, scale_backoffs and scale_growths are device tensors no stepping method reads; checkpoints hold them.  Both at
        their defaults: nothing is allocated and every call is the one made without the arguments.
        lr_schedule: None, or api.lr_schedule(...) / a dict of its arguments / a preset name ("nerf": x0.1 per 250k steps;
        "instant_ngp": x0.33 every 10k steps after 20k): the factor on lr and on the table's 10 lr, evaluated on the device from the
        step counter (librtxn: rtxn_optimizer_options, rtxn_optimizer_rate); current_lr() is its host restatement.
        weight_decay: AdamW's decoupled decay w -= lr_t weight_decay w, on the MLP only.  skip_nonfinite: a step whose gradients hold
        an Inf or a NaN leaves weights, moments and update counts as they are, clears the gradients and counts one up in
        skipped_steps (a device tensor, never read by the stepping methods); step_count advances all the same, so Adam's bias
        correction counts attempted steps.  A fixed loss scale stays what it is (loss_scale="dynamic" lowers it on every skipped step).  All three at
        their defaults (or a constant schedule without warm-up): nothing is allocated and every call is the one made without the
        arguments.  Configuration, not state, as loss is; checkpoints hold only the skipped count.
        distortion_weight: lambda_d of mip-NeRF 360's distortion regulariser (librtxn: rtxn_volrender_reg_train /
        rtxn_train_gradients_reg / rtxn_train_step_reg), in world distances along the ray (a lambda quoted for distances normalised to
        [0, 1] is divided by the cube's diagonal 2 sqrt(3)); mode "nerf" and the fused compositor only.  Its gradient is ~1e-7 per
        sample at lambda_d = 0.01, loss_scale 128 and 4096 rays, at the edge of the fp16 radiance gradients: raise loss_scale with it.
        Trainer.distortion holds L_r of every ray of the last batch.  0.0: nothing is allocated and every call is the one made
        without the argument.  Configuration, not state, as loss is.
        loss: "l2" (the reference's; every code path as without the argument), "l1", "huber" (loss_param: delta, default 0.1) or
        "relative_l2" (loss_param: epsilon, default 1e-2); opacity_weight: lambda of the alpha term lambda (A - alpha)^2, which fits
        the ray's opacity to the fourth channel of RGBA targets (librtxn: rtxn_volrender_loss_train /
        rtxn_train_gradients_loss / rtxn_train_step_loss).  Configuration, not state: checkpoints do not hold it.
        sample_jitter: draw the 32 samples of every segment at fresh positions inside their strata on every training step
        (SAMPLING_JITTER_WORLD; mode "nerf" only) instead of at the midpoints; rendering and the occupancy refresh stay
        at the midpoints.  jitter_seed: its seed (the rank is mixed in when data parallel).
        background: None (black, the reference's compositor), (r, g, b) -- train over that constant colour -- or "random":
        a fresh colour per ray and step (librtxn: rtxn_volrender_l2_train_ex / rtxn_train_gradients_ex /
        rtxn_train_step_ex).  Targets are [n, 3] or straight RGBA [n, 4] (composited over the ray's background in the kernel);
        "random" needs RGBA.  target_channels: the width of graph_targets for the captured / one-call steps (default 4 with
        "random", else 3).  background_seed: RANDOM's seed (the rank is mixed in when data parallel)."""
        self.R = grid_res
        self.dev = torch.device(device)
        self.occ = occupancy
        self.coarse = api.build_occupancy_mip(occupancy, grid_res) if (occupancy is not None and grid_res % 4 == 0) else None
        self.bricks = api.build_occupancy_bricks(occupancy, grid_res) if self.coarse is not None else None
        self.super_mip = api.build_occupancy_mip(self.coarse, grid_res // 4) if (self.coarse is not None and grid_res % 16 == 0) else None
        self.B = batch_rays
        self.mode = mode
        self.lr, self.loss_scale, self.density_scale = lr, loss_scale, density_scale
        self.step_count = 0
        self.occ_density = None    # refresh_occupancy(): the running maximum, its workspace and its device outputs, on first use
        self._occ_ws = self._occ_out = self._occ_step = None
        self._occ_seed = seed
        self._stage_ev = None     # list of (stage, start event, end event) while time_stages() is collecting
        self._init_background(background, background_seed, target_channels)      # refused before anything is allocated
        self._init_jitter(sample_jitter, jitter_seed)
        self._init_loss(loss, loss_param, opacity_weight)
        self._init_regularizer(distortion_weight)
        self._init_depth(depth_weight, depth_loss, depth_loss_param)
        self._init_scaler(loss_scale, max_grad_norm)
        self._init_ema(ema_decay)
        self._init_optimizer(lr_schedule, weight_decay, skip_nonfinite or self._scaler_cfg is not None)
        if ray_gradients and encoding != "hash":
            raise ValueError(f"Trainer: ray_gradients needs encoding='hash' (got {encoding!r}): the frequency and lean paths form no "
                             "d(encoding) to differentiate through")
        self.ray_gradients = bool(ray_gradients)
        self._pose = None          # attach_images(refine_poses=...): the per-image pose correction
        self._cams = None          # attach_images(refine_cameras=...): the intrinsics refinement
        self.image_set = None      # attach_images(): batches drawn on the device
        self.draw_count = 0        # batches drawn so far: host mirror of the device counter the draw is keyed on
        self._draw_step = None
        d = self.dev
        # ---- model -------------------------------------------------------------------------------
        self.encoding = encoding
        if encoding == "hash":
            self.hg = api.HashGrid(n_dir_freqs=n_dir_freqs, **(hashgrid or {}))
            E = self.hg.encoded_width()
            self.net = api.Network(n_neurons=n_neurons, n_hidden_layers=n_hidden_layers, n_encoded_features=E)
            g = torch.Generator().manual_seed(seed + 1)
            self.table_master = ((torch.rand(self.hg.n_params(), generator=g) * 2 - 1) * 1e-4).to(d)   # tcnn: U(-1e-4, 1e-4)
            self.table = self.table_master.half()
            self.table_m = torch.zeros_like(self.table_master)
            self.table_v = torch.zeros_like(self.table_master)
            # tiny-cuda-nn's Adam treats the table as "non-matrix" parameters: entries with a zero gradient are skipped and
            # each entry counts its own updates for the bias correction (librtxn: rtxn_adam_step_sparse).  Also the cheap
            # form -- a batch touches 0.2 .. 25 % of a hashed level.  RTXN_TABLE_ADAM=dense: every entry every step, global
            # step count (rounds 1-2; A/B).
            self.table_steps = torch.zeros(self.hg.n_params(), dtype=torch.int32, device=d)
            self.table_adam_sparse = os.environ.get("RTXN_TABLE_ADAM", "sparse") != "dense"
            self.dtable = torch.zeros_like(self.table_master)
            # The hashed levels' gradient lives in fp16 (dtable_h = parameters hashed_lo..): the scatter writes both features
            # of a corner with one packed fp16 atomic (tiny-cuda-nn's grid gradient is __half2 too), the data-parallel
            # exchange sends it as it is, and it is widened into dtable[hashed_lo:] for Adam.  The densely stored leading
            # levels (thousands of contributions per entry) stay fp32.  RTXN_HASH_GRAD_FP16=0: everything fp32.
            self.hashed_lo = self.hg.hashed_offset()
            self.hash_fp16 = (self.hg.cfg.n_features == 2 and self.hashed_lo < self.hg.n_params()
                              and os.environ.get("RTXN_HASH_GRAD_FP16", "1") != "0")
            self.dtable_h = (torch.zeros(self.hg.n_params() - self.hashed_lo, dtype=torch.float16, device=d)
                             if self.hash_fp16 else None)
        else:
            self.hg = None
            self.net = api.Network(n_neurons=n_neurons, n_hidden_layers=n_hidden_layers)
            E = self.net.encoded_width()
        self.E = E
        self.master = self.net.initialize_params(seed).to(d)       # fp32 master (main.cu:328-349)
        self.params = self.master.half()                           # fp16 params
        self.adam_m = torch.zeros_like(self.master)
        self.adam_v = torch.zeros_like(self.master)
        self.dparams = torch.zeros_like(self.master)
        self.net.set_params(self.params)
        # optimizer options: the schedule's factor, the guard words, and the eager step's device counter and rates (the captured
        # and the one-call step have their own counters); nothing without options
        self._opt = self._opt_guard = self._opt_step = self._opt_lr = None
        if self._opt_active:
            self._opt_factor = torch.ones(1, device=d)
            self._opt_guard = torch.zeros(4, dtype=torch.int32, device=d)
            self._opt = api.optimizer_options(self._schedule, self.weight_decay, self.skip_nonfinite, self._opt_factor, self._opt_guard)
            self._opt_step = torch.zeros(1, dtype=torch.int32, device=d)
            self._opt_step_host = 0
            self._opt_lr = torch.zeros(2, device=d)
        # the loss scaler: its eight state words, the statistics kernel's per-block sums, and the struct over both
        self._scaler = self._scaler_state = self._scaler_ws = None
        if self._scaler_cfg is not None:
            c = self._scaler_cfg
            self._scaler_state = api.loss_scaler_state_tensor(c, device=d)
            self._scaler_ws = api.loss_scaler_workspace(device=d)
            self._scaler = api.loss_scaler(c.init_scale, c.growth, c.backoff, c.growth_interval, c.min_scale, c.max_scale, c.max_grad_norm,
                                           state=self._scaler_state, partials=self._scaler_ws)
        # the weight EMA: four state words, the accumulators, the table's stamps under the sparse rule, and the struct over them;
        # the model and table sync_ema() fills are made on first use
        self._ema = self._ema_state = self.ema_mlp = self.ema_table = self.ema_stamps = None
        self._ema_net = self._ema_table16 = None
        if self.ema_decay is not None:
            self._ema_state = torch.zeros(4, dtype=torch.int32, device=d)
            self.ema_mlp = torch.zeros_like(self.master)
            if encoding == "hash":
                self.ema_table = torch.zeros_like(self.table_master)
                self.ema_stamps = torch.zeros_like(self.table_steps) if self.table_adam_sparse else None
            self._ema = api.weight_ema(self.ema_decay, self._ema_state, self.ema_mlp, self.ema_table, self.ema_stamps)
        # 64-wide models (configs[2]): forward without saved activations + ONE fused backward kernel that recomputes them and
        # keeps every weight gradient on the chip (librtxn: mlp_bwd_fused64_kernel).  RTXN_TRAIN_RECOMPUTE=0 selects the
        # three-kernel path (saved activations, dgrad chain, weight-gradient GEMM) for A/B runs.
        self.recompute = self.net.recompute_supported() and os.environ.get("RTXN_TRAIN_RECOMPUTE", "1") != "0"
        # launchSampler folded into the encoders / the hash scatter (they form the samples from the packed segments): the
        # float[S][5] samples and the separate sampler launch exist only for teacher rendering (render_rays(radiance_fn)) and
        # for tests (materialize_samples()).  RTXN_TRAIN_FOLD_SAMPLER=0: the reference's stage order, sampler first.
        self.fold_sampler = os.environ.get("RTXN_TRAIN_FOLD_SAMPLER", "1") != "0"
        # "nerf" mode: compositor forward + L2 + compositor backward as one launch (RTXN_TRAIN_FUSE_COMPOSITOR=0: three)
        self.fuse_compositor = os.environ.get("RTXN_TRAIN_FUSE_COMPOSITOR", "1") != "0"
        # The backward visits only the segments that carry a loss gradient (librtxn: rtxn_live_segments; most of a NeRF batch
        # lies behind the first surface, where dL/d(radiance) is exactly 0).  A column tile of the backward kernels is one
        # segment, so a block tile can be any eight of them.  Needs the folded sampler.  RTXN_TRAIN_LIVE_SEGMENTS=0: every segment.
        self.live_segments = self.fold_sampler and os.environ.get("RTXN_TRAIN_LIVE_SEGMENTS", "1") != "0"
        # Saved-activation models (128 wide, or RTXN_TRAIN_RECOMPUTE=0) in "nerf" mode: the forward of a step runs OUTPUTS-ONLY over
        # the whole batch, and the activations are saved afterwards for the live segments alone (rtxn_mlp_train_forward_live) --
        # the full saving forward is HBM-bound on activations of which 70-90 % are never read.  ("compat" mode: the reference's
        # backward has no transmittance factor, every segment is live, one saving pass is the cheaper form.)
        # RTXN_TRAIN_TWO_PASS=0: one saving pass over everything.
        # The reference's own model (8 x 128, 112 encoded features): the LEAN path (librtxn: rtxn_mlp_train_forward_lean /
        # _backward_lean) -- the forward keeps outputs + sign masks only, the weight gradient recomputes the activations from the
        # encoding: 5.1 instead of 8.8 KB moved per sample and half the workspace.  RTXN_TRAIN_LEAN=0: the saved-activation path (A/B).
        self.lean = (not self.recompute and encoding != "hash" and self.net.lean_supported()
                     and os.environ.get("RTXN_TRAIN_LEAN", "1") != "0")
        # ... and with the reference's Composite-Frequency(3 x 10, 2 x 12) encoding the sampler and the encoder are folded into both lean
        # kernels (rtxn_mlp_train_forward_lean_segments / _backward_lean_segments): no encoder launch, encT never written -- the same
        # values bit for bit.  RTXN_TRAIN_LEAN_FUSED=0: the staged encoder (A/B; librtxn's one-call step reads the same switch).
        self.lean_fused = (self.lean and self.fold_sampler and self.net.lean_fused_supported()
                           and os.environ.get("RTXN_TRAIN_LEAN_FUSED", "1") != "0")
        self.two_pass = (not self.recompute and not self.lean and self.live_segments and mode == "nerf"
                         and os.environ.get("RTXN_TRAIN_TWO_PASS", "1") != "0")
        # ---- per-step buffers at capacity ---------------------------------------------------------
        B = batch_rays
        self.max_segments = int(max_segments) if max_segments else 64 * B
        M, K = self.max_segments, api.NUM_SAMPLES_PER_SEGMENT
        self.view_dirs = torch.empty((B, 2), device=d)
        self.num_hits = torch.empty(B, dtype=torch.int32, device=d)
        self.indices = torch.empty(B, dtype=torch.int32, device=d)
        self.num_stored = torch.empty(B, dtype=torch.int32, device=d)   # segments actually written per ray (= num_hits unless cut off)
        self.truncated_steps = 0
        self.total = torch.zeros(1, dtype=torch.int32, device=d)
        # a batch is a small launch: several lanes walk each ray (bit-identical segments, shorter critical path)
        self.sub_rays = api.auto_sub_rays(B)              # for a full batch_rays launch; smaller launches take more lanes per ray
        self.sub_hits = torch.zeros(max(api.auto_sub_rays(n) * n for n in {min(B, t) for t in (11_999, 29_999, 119_999, 299_999, B)}),
                                    dtype=torch.int32, device=d)           # the largest lanes x rays of any launch of <= B rays
        self.scan_ws = torch.empty((api._lib.lib().rtxn_scan_workspace_bytes(B) + 3) // 4, dtype=torch.int32, device=d)
        self.start = torch.empty((M, 3), device=d)
        self.end = torch.empty((M, 3), device=d)
        self.seg_view = torch.empty((M, 2), device=d)      # (theta, phi) of each segment's ray, written by the traversal
        self.samples = torch.empty((M * K, 5), device=d)
        self.t_vals = torch.empty(M * K, device=d)
        Sp = api.padded_samples(M * K)
        self.encT = torch.empty((E, Sp), dtype=torch.float16, device=d)
        self.dencT = torch.empty((E, Sp), dtype=torch.float16, device=d) if encoding == "hash" else None
        if self.recompute:
            self.ws = None
        elif self.lean:
            self.ws = self.net.train_lean_workspace(M * K, device=d)                        # dZ | masks
        else:
            self.ws = self.net.train_workspace(M * K, device=d)                             # saved activations | dZ | masks
        self.out = torch.empty((M * K, 16), dtype=torch.float16, device=d)
        self.radiance = torch.empty((M * K, 4), device=d)
        self.dout = torch.empty((M * K, 4), dtype=torch.float16, device=d)
        self.live_ws = api.live_segments_workspace(M, device=d) if self.live_segments else None
        self.pixels = torch.empty((B, 3), device=d)
        self.loss_grads = torch.empty((B, 3), dtype=torch.float16, device=d)
        self.loss = torch.zeros(1, device=d)
        # the alpha term's per-ray opacities, written by the loss compositor (deterministic mode sums the loss from them)
        self.opacity = torch.zeros(B, device=d) if self.opacity_weight > 0.0 else None
        self._loss = (api.train_loss(self.loss_kind, self.loss_param, self.opacity_weight, self.opacity)
                      if (self.loss_kind != "l2" or self.opacity_weight > 0.0) else None)
        # the distortion regulariser: the segments' entry / exit distances, written by the traversal's write pass, and L_r per ray
        self.t_start = self.t_end = self.distortion = self._reg = None
        if self.distortion_weight > 0.0:
            self.t_start, self.t_end = torch.zeros(M, device=d), torch.zeros(M, device=d)
            self.distortion = torch.zeros(B, device=d)
            self._reg = api.train_regularizer(self.distortion_weight, self.t_start, self.t_end, self.distortion)
        # the ray gradients: the segments' distances (shared with the regulariser), their end-point gradients, and dL/d(ray)
        self.dstart = self.dend = self.rays_o_grad = self.rays_d_grad = self._rays = None
        if self.ray_gradients:
            if self.t_start is None:
                self.t_start, self.t_end = torch.zeros(M, device=d), torch.zeros(M, device=d)
            self.dstart, self.dend = torch.zeros((M, 3), device=d), torch.zeros((M, 3), device=d)
            self.rays_o_grad, self.rays_d_grad = torch.zeros((B, 3), device=d), torch.zeros((B, 3), device=d)
            self._rays = api.ray_gradients(self.t_start, self.t_end, self.dstart, self.dend, self.rays_o_grad, self.rays_d_grad)
        # the depth term: the rays' targets, D_r and l(e_r) per ray, over the same segment distances
        self.depth_targets = self.depth = self.depth_loss = self._depth = None
        if self.depth_weight > 0.0:
            if self.t_start is None:
                self.t_start, self.t_end = torch.zeros(M, device=d), torch.zeros(M, device=d)
            self.depth_targets, self.depth, self.depth_loss = torch.zeros(B, device=d), torch.zeros(B, device=d), torch.zeros(B, device=d)
            self._depth = self._depth_struct(self.depth_targets, self.t_start, self.t_end)
        # data parallel (world > 1): the MLP gradient's all-reduce is issued from inside gradients(), right behind the MLP
        # backward, and runs beside the hash scatter; the hashed levels go through dp.Half2GradExchange (lists where a level
        # is sparse, RTXN_DP_SPARSE=0: always the dense fp16 level)
        self._dp_pending = None
        self._dp_table = None
        self.dp_sparse = os.environ.get("RTXN_DP_SPARSE", "1") != "0"         # "force": lists for every level (tests)
        # deterministic=True (or RTXN_DETERMINISTIC=1): every cross-workgroup gradient sum in 64-bit fixed point instead of float
        # atomics (librtxn: rtxn_set_deterministic_workspace): two runs, or two ranks, of the same steps end with identical bits.
        # The library's switch is process-wide, so every stepping method re-asserts this trainer's choice first (_det_select).
        self.deterministic = (os.environ.get("RTXN_DETERMINISTIC", "0") == "1") if deterministic is None else bool(deterministic)
        self._det_mlp = api.deterministic_shadow(self.master.numel(), device=d) if self.deterministic else None
        self._det_table = (api.deterministic_shadow(self.table_master.numel(), device=d)
                           if (self.deterministic and encoding == "hash") else None)
        # A trainer collected while its shadows are still the registered ones switches the library back to the float atomics:
        # direct backward calls made afterwards (Network.train_backward*, HashGrid.backward*, api.train_gradients) run in
        # default mode, not into this trainer's shadows.
        if self.deterministic:
            weakref.finalize(self, api.release_deterministic, self._det_mlp, self._det_table).atexit = False

    # ------------------------------------------------------------------------------------------
    def _init_background(self, background, seed, target_channels):
        if isinstance(background, str) and background != "random":
            raise ValueError(f"Trainer: background {background!r}: None, (r, g, b) or 'random'")
        if background is not None and not isinstance(background, str):
            background = tuple(float(v) for v in background)
            if len(background) != 3:
                raise ValueError(f"Trainer: background {background!r}: three floats")
        if background is not None and self.mode != "nerf":
            raise ValueError("Trainer: a background needs mode='nerf': the compat compositor's backward is not the gradient of its "
                             "forward, so it has no background form")
        if background is not None and os.environ.get("RTXN_TRAIN_FUSE_COMPOSITOR", "1") == "0":
            raise ValueError("Trainer: a background needs the fused training compositor (RTXN_TRAIN_FUSE_COMPOSITOR=0 selects the "
                             "three-launch compositor, which has no background form)")
        random = background == "random"
        tc = int(target_channels) if target_channels is not None else (4 if random else 3)
        if tc not in (3, 4) or (random and tc == 3) or (background is None and tc == 4):
            raise ValueError(f"Trainer: target_channels = {tc} with background {background!r} (3 or 4; 'random' needs 4 (RGBA), "
                             "RGBA needs a background)")
        self.background, self.background_seed, self.target_channels = background, int(seed), tc
        # RANDOM hashes the step number from a DEVICE int: this one for step(), the captured counter for step_captured(),
        # the optimizer's own for step_entry() -- the same step number draws the same backgrounds on all three paths
        self._bg_step = torch.zeros(1, dtype=torch.int32, device=self.dev) if random else None
        self._bg_step_host = 0

    def _init_loss(self, kind, param, opacity_weight):
        if kind not in api.LOSS_KINDS:
            raise ValueError(f"Trainer: loss {kind!r}: one of {sorted(api.LOSS_KINDS)}")
        lam = float(opacity_weight)
        if param is not None and kind in ("huber", "relative_l2") and not (float(param) > 0.0 and np.isfinite(float(param))):
            raise ValueError(f"Trainer: loss_param = {param!r}: {kind} needs a finite value > 0")
        if not (lam >= 0.0 and np.isfinite(lam)):
            raise ValueError(f"Trainer: opacity_weight = {opacity_weight!r} (finite, >= 0)")
        if lam > 0.0 and self.target_channels != 4:
            raise ValueError("Trainer: opacity_weight > 0 fits the opacity to the alpha of RGBA targets: it needs a background and "
                             "target_channels=4 (mode='nerf')")
        self.loss_kind, self.loss_param, self.opacity_weight = kind, (float(param) if param is not None else None), lam

    def _init_regularizer(self, distortion_weight):
        lam = float(distortion_weight)
        if not (lam >= 0.0 and np.isfinite(lam)):
            raise ValueError(f"Trainer: distortion_weight = {distortion_weight!r} (finite, >= 0)")
        if lam > 0.0 and self.mode != "nerf":
            raise ValueError("Trainer: distortion_weight > 0 needs mode='nerf': the regulariser lives in the fused NeRF compositor "
                             "and measures world distances, which mode='compat' does not sample")
        if lam > 0.0 and os.environ.get("RTXN_TRAIN_FUSE_COMPOSITOR", "1") == "0":
            raise ValueError("Trainer: distortion_weight > 0 needs the fused training compositor (RTXN_TRAIN_FUSE_COMPOSITOR=0 selects "
                             "the three-launch compositor, which has no regulariser)")
        self.distortion_weight = lam

    def _init_depth(self, depth_weight, kind, param):
        lam = float(depth_weight)
        if not (lam >= 0.0 and np.isfinite(lam)):
            raise ValueError(f"Trainer: depth_weight = {depth_weight!r} (finite, >= 0)")
        if kind not in api.DEPTH_LOSS_KINDS:
            raise ValueError(f"Trainer: depth_loss {kind!r}: one of {sorted(api.DEPTH_LOSS_KINDS)}")
        if param is not None and kind == "huber" and not (float(param) > 0.0 and np.isfinite(float(param))):
            raise ValueError(f"Trainer: depth_loss_param = {param!r}: huber needs a finite value > 0")
        if lam > 0.0 and self.mode != "nerf":
            raise ValueError("Trainer: depth_weight > 0 needs mode='nerf': the depth term lives in the fused NeRF compositor and "
                             "measures world distances, which mode='compat' does not sample")
        if lam > 0.0 and os.environ.get("RTXN_TRAIN_FUSE_COMPOSITOR", "1") == "0":
            raise ValueError("Trainer: depth_weight > 0 needs the fused training compositor (RTXN_TRAIN_FUSE_COMPOSITOR=0 selects the "
                             "three-launch compositor, which has no depth term)")
        self.depth_weight, self.depth_loss_kind = lam, kind
        self.depth_loss_param = float(param) if param is not None else None

    def _depth_struct(self, target, t_start, t_end):
        """api.train_depth over a target buffer and the segment distances of the buffer set it is trained on"""
        return api.train_depth(self.depth_weight, self.depth_loss_kind, self.depth_loss_param, target, t_start, t_end, self.depth,
                               self.depth_loss)

    def _init_ema(self, ema_decay):
        """the library's own rule (rtxn_weight_ema_check), before anything is allocated"""
        self.ema_decay = None
        if ema_decay is None:
            return
        try:
            self.ema_decay = float(api.weight_ema(float(ema_decay)).decay)
        except (api._lib.RtxnError, TypeError, ValueError) as e:
            raise ValueError(f"Trainer: ema_decay = {ema_decay!r}: {e}") from None

    @property
    def ema_updates(self):
        """device int32[1]: applied updates the average has seen (None without ema_decay)"""
        return None if self._ema_state is None else self._ema_state[0:1]

    def ema_parameters(self):
        """(mlp fp32, table fp32 | None): the debiased average of the weights now (rtxn_ema_weights), in the layouts of master and
        table_master; before the first applied update, the weights themselves.  Reads the training state, changes none of it."""
        if self._ema is None:
            raise RuntimeError("ema_parameters: this trainer was made without ema_decay")
        mlp = torch.empty_like(self.master)
        api.ema_weights(self.master, self.ema_mlp, None, self._ema_state, self.ema_decay, out_f32=mlp)
        table = None
        if self.encoding == "hash":
            table = torch.empty_like(self.table_master)
            api.ema_weights(self.table_master, self.ema_table, self.ema_stamps, self._ema_state, self.ema_decay, out_f32=table)
        return mlp, table

    def sync_ema(self):
        """Refresh the averaged model render_pipeline(weights="ema") draws: a second model handle and a second fp16 table, filled
        from the read-out.  The handle goes through set_params, so the frequency model's fused inference packing is refreshed too.
        The live model, its table and the training state are only read."""
        if self._ema is None:
            raise RuntimeError("sync_ema: this trainer was made without ema_decay")
        if self._ema_net is None:
            c = self.net.cfg
            self._ema_net = api.Network(n_neurons=c.n_neurons, n_hidden_layers=c.n_hidden_layers, n_pos_freqs=c.n_pos_freqs,
                                        n_dir_freqs=c.n_dir_freqs, n_pos_dims=c.n_pos_dims, n_dir_dims=c.n_dir_dims,
                                        n_output_dims=c.n_output_dims, output_activation=c.output_activation,
                                        n_encoded_features=c.n_encoded_features)
            self._ema_params16 = torch.empty_like(self.params)
            if self.encoding == "hash":
                self._ema_table16 = torch.empty_like(self.table)
        api.ema_weights(self.master, self.ema_mlp, None, self._ema_state, self.ema_decay, out_f16=self._ema_params16)
        self._ema_net.set_params(self._ema_params16)
        if self.encoding == "hash":
            api.ema_weights(self.table_master, self.ema_table, self.ema_stamps, self._ema_state, self.ema_decay, out_f16=self._ema_table16)

    def _init_scaler(self, loss_scale, max_grad_norm):
        """loss_scale / max_grad_norm -> self._scaler_cfg (a struct without buffers, or None) and self.loss_scale (the fixed or the
        initial scale); the library's own rules (rtxn_loss_scaler_check), before anything is allocated"""
        try:
            mgn = 0.0 if max_grad_norm is None else float(max_grad_norm)
            if not (np.isfinite(mgn) and mgn >= 0.0):
                raise ValueError("max_grad_norm must be finite and >= 0")
            if isinstance(loss_scale, str):
                if loss_scale != "dynamic":
                    raise ValueError("a float, 'dynamic' or api.loss_scaler(...)")
                cfg = api.loss_scaler()
            elif isinstance(loss_scale, (dict, api._lib.LossScaler)):
                cfg = api.loss_scaler(loss_scale)
            elif mgn > 0.0:       # a fixed scale through the scaled path: nothing moves it
                ls = float(loss_scale)
                cfg = api.loss_scaler(init_scale=ls, growth=1.0, backoff=0.5, growth_interval=1, min_scale=ls, max_scale=ls)
            else:
                self._scaler_cfg, self.loss_scale = None, loss_scale
                return
            if max_grad_norm is not None:
                cfg = api.loss_scaler(cfg.init_scale, cfg.growth, cfg.backoff, cfg.growth_interval, cfg.min_scale, cfg.max_scale, mgn)
        except (api._lib.RtxnError, TypeError, ValueError) as e:
            raise ValueError(f"Trainer: loss_scale = {loss_scale!r}, max_grad_norm = {max_grad_norm!r}: {e}") from None
        if self.mode != "nerf":
            raise ValueError("Trainer: a dynamic loss scale / max_grad_norm needs mode='nerf': the scale is read from device memory by "
                             "the fused NeRF compositor alone")
        if os.environ.get("RTXN_TRAIN_FUSE_COMPOSITOR", "1") == "0":
            raise ValueError("Trainer: a dynamic loss scale / max_grad_norm needs the fused training compositor "
                             "(RTXN_TRAIN_FUSE_COMPOSITOR=0 selects the three-launch compositor, which takes the scale by value)")
        self._scaler_cfg, self.loss_scale = cfg, float(cfg.init_scale)

    def _scaler_word(self, k, as_float=False):
        if self._scaler_state is None:
            return None
        w = self._scaler_state[k:k + 1]
        return w.view(torch.float32) if as_float else w

    @property
    def loss_scale_now(self):
        """device float32[1]: the scale the NEXT compositor launch reads (None without a scaler)"""
        return self._scaler_word(0, True)

    @property
    def grad_norm(self):
        """device float32[1]: the last clean step's unscaled total gradient norm (None without a scaler)"""
        return self._scaler_word(6, True)

    @property
    def clipped_steps(self):
        """device int32[1]: steps whose gradient was clipped so far (None without a scaler)"""
        return self._scaler_word(5)

    @property
    def scale_backoffs(self):
        """device int32[1]: times the scale was lowered = steps skipped under the scaler (None without a scaler)"""
        return self._scaler_word(3)

    @property
    def scale_growths(self):
        """device int32[1]: times the scale was raised (None without a scaler)"""
        return self._scaler_word(4)

    def _init_optimizer(self, lr_schedule, weight_decay, skip_nonfinite):
        """the library's own rules (rtxn_optimizer_options_check), before anything is allocated"""
        try:
            self._schedule = api.lr_schedule(lr_schedule) if lr_schedule is not None else None
            self.weight_decay, self.skip_nonfinite = float(weight_decay), bool(skip_nonfinite)
            api.optimizer_options_check(api.optimizer_options(self._schedule, self.weight_decay, self.skip_nonfinite))
        except (api._lib.RtxnError, TypeError, ValueError) as e:
            raise ValueError(f"Trainer: lr_schedule = {lr_schedule!r}, weight_decay = {weight_decay!r}: {e}") from None
        sch = self._schedule
        scheduled = sch is not None and (sch.kind != api.LR_CONSTANT or sch.warmup_steps > 0)
        # the weight EMA's steps take the options path with whatever is switched on, nothing included: the rate kernel counts its updates
        self._opt_active = scheduled or self.weight_decay > 0.0 or self.skip_nonfinite or self.ema_decay is not None
        if not scheduled:
            self._schedule = None

    @property
    def skipped_steps(self):
        """device int32[1]: steps the non-finite guard skipped so far (None without optimizer options)"""
        return None if self._opt_guard is None else self._opt_guard[1:2]

    def current_lr(self):
        """The MLP's scheduled rate lr_t of the NEXT update (the table's is 10 x): lr times the host restatement of the schedule
        (rtxn_lr_schedule_factor) at step_count + 1, without Adam's bias correction."""
        f = 1.0 if self._schedule is None else api.lr_schedule_factor(self._schedule, self.step_count + 1)
        return float(np.float32(self.lr) * np.float32(f))

    def _reg_t(self, st=None):
        """the write pass's t_start / t_end arguments: the regulariser's and the ray gradients' buffers (of buffer set st), or nothing"""
        if self.t_start is None:
            return {}
        return dict(t_start=self.t_start if st is None else st["t_start"], t_end=self.t_end if st is None else st["t_end"])

    def _init_jitter(self, sample_jitter, seed):
        if sample_jitter and self.mode != "nerf":
            raise ValueError("Trainer: sample_jitter needs mode='nerf': the jittered sampler writes step lengths (MIDPOINT_WORLD's "
                             "t_vals), which the compat compositor does not take")
        self.sample_jitter, self.jitter_seed = bool(sample_jitter), int(seed)
        # the step number is hashed from a DEVICE int, kept as the background's is: this one for step(), the captured counter for
        # step_captured(), the optimizer's own for step_entry() -- the same step number draws the same offsets on all three paths
        self._jit_step = torch.zeros(1, dtype=torch.int32, device=self.dev) if self.sample_jitter else None
        self._jit_step_host = 0

    def _jitter(self, step):
        """api.sample_jitter for this trainer, `step` the device int32 counter (None: 0 / opt.step); None when jitter is off."""
        if not self.sample_jitter:
            return None
        seed = self.jitter_seed
        if _world() > 1:                        # every rank draws its own offsets
            seed = (seed + 0x632BE5AB * dist.get_rank()) & 0xFFFFFFFF
        return api.sample_jitter(seed=seed, step=step)

    def _bg(self, step, n_channels):
        """api.train_background for this trainer's background, `step` the device int32 counter (None: 0 / opt.step)."""
        if self.background is None:
            return None
        seed = self.background_seed
        if _world() > 1:                        # every rank draws its own backgrounds
            seed = (seed + 0x632BE5AB * dist.get_rank()) & 0xFFFFFFFF
        return api.train_background(self.background, seed=seed, step=step, target_channels=n_channels)

    # ------------------------------------------------------------------------------------------ device batches
    def attach_images(self, image_set, draw_seed=0, refine_poses=None, refine_cameras=None):
        """Draw this trainer's batches on the device from the resident frames of an api.ImageSet (librtxn: rtxn_draw_batch,
        DESIGN 5.10): step_images(), capture_step(draw=True) and entry_args(draw=True) then need no rays or targets from the
        caller.  The set's channel count must be the trainer's target width (3, or 4 = straight RGBA over its background).
        Batch k of the sequence is a pure function of (draw_seed, k) -- the rank is mixed into the seed when data parallel --
        and k is a DEVICE int32 counter of the batches drawn so far, advanced stream-ordered by one behind every draw: it is
        not the optimizer's step, so batch k is the same batch on all three stepping paths, with or without prefetch.
        self.draw_count mirrors it on the host (checkpoints keep it); self.drawn holds (image, y*W + x) of the last draw.
        A graph captured with draw=True and the struct of entry_args(draw=True) hold the counter's, the frames' and the
        poses' addresses, so once either exists another set cannot be attached: build a new Trainer for it.
        A set with cameras (api.ImageSet(cameras=)) draws every batch through rtxn_draw_batch_cameras on all three
        paths -- same (image, pixel) and targets, the ray from the image's camera -- and the address rule covers its camera tensor.
        refine_poses: None, True, or a dict of lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15 (a trainer built with ray_gradients=True;
        DESIGN 5.16; librtxn: rtxn_pose_refinement): a 6-DoF correction (omega, tau) per image, optimised on the device inside
        step_images(), step_captured() (capture_step(draw=True)) and step_entry() (entry_args(draw=True)) behind the optimizer, by
        Adam on the gradient the batch's rays carry.  The set's poses are rewritten IN PLACE as (R(omega) R0 | t0 + tau) against a
        clone of the poses as attached, so the next draw generates its rays from the refined poses with nothing else to change.
        pose_delta [N, 6], pose_updates [N] and pose_skipped [1] are device tensors no stepping method reads; refined_poses()
        returns the poses, reset_poses() restores the attached ones; checkpoints hold delta, moments, counts and the skipped count.
        An image without a ray in the batch keeps its moments and count; a step the non-finite guard skips moves nothing.
        refine_cameras: None, True, or a dict of lr_focal, lr_center, lr_distortion, max_log_focal, max_center, max_distortion,
        beta1, beta2, eps (defaults api.CAMERA_REFINE_DEFAULTS; librtxn: rtxn_camera_refinement): the rows of the
        set's cameras (a set built with cameras=; a trainer built with ray_gradients=True; single GPU) optimised on the same three
        paths, behind the optimizer and beside refine_poses -- pose gradient, camera gradient, pose step, camera step.  Three
        groups with a rate each (0 freezes the group): fx, fy as fx0 exp(delta), cx, cy in pixels, the distortion coefficients
        the model has; max_* clamp |delta|.  The CameraSet's tensor is rewritten IN PLACE against a clone of the rows as
        attached, so the next draw reads the refined rows.  camera_delta [n_cameras, 10], camera_updates [n_cameras] and
        camera_skipped [1] are device tensors no stepping method reads; refined_cameras() returns a copy of the rows,
        reset_cameras() restores the attached ones, check_cameras() runs the host's float64 invertibility check on the live rows
        (the clamps are safety rails, not that guarantee); checkpoints hold delta, moments, counts and the skipped count.
        A CameraSet shared with a held-out ImageSet is scored by evaluate() with the refined rows: the tensor is the same."""
        if getattr(self, "_g_draw", False) or getattr(self, "_entry_draw", None) is not None:
            raise RuntimeError("Trainer.attach_images: a captured graph or an entry struct of this trainer already draws from the attached "
                               "set (capture_step(draw=True) / entry_args(draw=True) keep its addresses); build a new Trainer")
        c = int(image_set.channels)
        if c != self.target_channels:           # refused before anything is allocated
            raise ValueError(f"Trainer.attach_images: a {c}-channel image set for a trainer that takes {self.target_channels}-channel targets" +
                             (" (RGBA frames need a background and target_channels=4)" if c == 4 else
                              " (this trainer composites straight RGBA targets over its background: load the frames with their alpha)"))
        cfg = None
        if refine_poses is not None and refine_poses is not False:      # refused before anything is allocated
            if not self.ray_gradients:
                raise ValueError("Trainer.attach_images: refine_poses needs a trainer built with ray_gradients=True")
            if _world() > 1:
                raise ValueError("Trainer.attach_images: refine_poses is single-GPU (every rank would move its own copy of the poses); "
                                 "ray_gradients alone is per rank and allowed")
            if refine_poses is not True and not isinstance(refine_poses, dict):
                raise ValueError(f"Trainer.attach_images: refine_poses = {refine_poses!r}: None, True or a dict of lr, beta1, beta2, eps")
            cfg = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15)
            extra = set(refine_poses) - set(cfg) if isinstance(refine_poses, dict) else set()
            if extra:
                raise ValueError(f"Trainer.attach_images: refine_poses has no {sorted(extra)} (lr, beta1, beta2, eps)")
            cfg.update(refine_poses if isinstance(refine_poses, dict) else {})
            try:
                api.pose_refinement(int(image_set.n_images), **{k: float(v) for k, v in cfg.items()})
            except (api._lib.RtxnError, TypeError, ValueError) as e:
                raise ValueError(f"Trainer.attach_images: refine_poses = {refine_poses!r}: {e}") from None
        ccfg = None
        if refine_cameras is not None and refine_cameras is not False:  # refused before anything is allocated
            if not self.ray_gradients:
                raise ValueError("Trainer.attach_images: refine_cameras needs a trainer built with ray_gradients=True")
            if getattr(image_set, "cameras", None) is None:
                raise ValueError("Trainer.attach_images: refine_cameras needs an image set built with cameras= (api.camera_set): "
                                 "the set's own pinhole has no rows to refine")
            if _world() > 1:
                raise ValueError("Trainer.attach_images: refine_cameras is single-GPU (every rank would move its own copy of the rows)")
            if refine_cameras is not True and not isinstance(refine_cameras, dict):
                raise ValueError(f"Trainer.attach_images: refine_cameras = {refine_cameras!r}: None, True or a dict of "
                                 f"{', '.join(api.CAMERA_REFINE_DEFAULTS)}")
            ccfg = dict(api.CAMERA_REFINE_DEFAULTS)
            extra = set(refine_cameras) - set(ccfg) if isinstance(refine_cameras, dict) else set()
            if extra:
                raise ValueError(f"Trainer.attach_images: refine_cameras has no {sorted(extra)} ({', '.join(ccfg)})")
            ccfg.update(refine_cameras if isinstance(refine_cameras, dict) else {})
            try:
                ccfg = {k: float(v) for k, v in ccfg.items()}
                api.camera_refinement(image_set.cameras.model, image_set.cameras.n_cameras, int(image_set.width), **ccfg)
            except (api._lib.RtxnError, TypeError, ValueError) as e:
                raise ValueError(f"Trainer.attach_images: refine_cameras = {refine_cameras!r}: {e}") from None
        if self.depth_weight > 0.0 and getattr(image_set, "depth", None) is None:
            raise ValueError("Trainer.attach_images: depth_weight > 0 needs an image set with depth maps (api.ImageSet(depth=...))")
        if not image_set.images.is_cuda:
            raise api._lib.RtxnError("Trainer.attach_images: the image set must live on the device (librtxn has no CPU path)")
        d = self.dev
        self.image_set, self.draw_seed = image_set, int(draw_seed)
        self._draw_step = torch.full((1,), self.draw_count, dtype=torch.int32, device=d)
        self.draw_rays_o = torch.empty((self.B, 3), device=d)
        self.draw_rays_d = torch.empty((self.B, 3), device=d)
        self.draw_targets = torch.empty((self.B, c), device=d)
        self.drawn = torch.zeros((self.B, 2), dtype=torch.int32, device=d)
        self._pose = None
        if cfg is not None:
            N = int(image_set.n_images)
            self.poses0 = image_set.poses.clone()
            self.pose_delta, self._pose_m, self._pose_v = (torch.zeros((N, 6), device=d) for _ in range(3))
            self.pose_updates = torch.zeros(N, dtype=torch.int32, device=d)
            self.pose_skipped = torch.zeros(1, dtype=torch.int32, device=d)
            self._pose_grad = torch.zeros((N, 8), device=d)
            self._pose = api.pose_refinement(N, **{k: float(v) for k, v in cfg.items()}, poses0=self.poses0, poses=image_set.poses,
                                             delta=self.pose_delta, m=self._pose_m, v=self._pose_v, steps=self.pose_updates,
                                             grad=self._pose_grad, skip=None if self._opt_guard is None else self._opt_guard[2:3],
                                             skipped=self.pose_skipped, drawn=self.drawn)
        self._cams = None
        if ccfg is not None:
            cams = image_set.cameras
            K = int(cams.n_cameras)
            self.cameras0 = cams.params.clone()
            self.camera_delta, self._cam_m, self._cam_v = (torch.zeros((K, api.CAMERA_DELTA), device=d) for _ in range(3))
            self.camera_updates = torch.zeros(K, dtype=torch.int32, device=d)
            self.camera_skipped = torch.zeros(1, dtype=torch.int32, device=d)
            self._cam_grad = torch.zeros((K, 12), device=d)
            self._cam_terms = torch.zeros((self.B, 12), device=d)
            self._cams = api.camera_refinement(cams.model, K, int(image_set.width), **ccfg, params0=self.cameras0, params=cams.params,
                                               delta=self.camera_delta, m=self._cam_m, v=self._cam_v, steps=self.camera_updates,
                                               grad=self._cam_grad, terms=self._cam_terms,
                                               skip=None if self._opt_guard is None else self._opt_guard[2:3],
                                               skipped=self.camera_skipped, drawn=self.drawn, poses=image_set.poses)
        return self

    def refined_cameras(self):
        """[n_cameras, 12]: the attached set's camera rows as the refinement has left them (a copy)"""
        if self.image_set is None or getattr(self.image_set, "cameras", None) is None:
            raise RuntimeError("refined_cameras: attach_images() with a set built with cameras= first")
        return self.image_set.cameras.params.clone()

    def reset_cameras(self):
        """Zero the intrinsics correction, its moments and counts, and restore the rows as attached."""
        if self._cams is None:
            raise RuntimeError("reset_cameras: attach_images(refine_cameras=...) first")
        for t in self._camera_arrays().values():
            t.zero_()
        self.image_set.cameras.params.copy_(self.cameras0)

    def check_cameras(self):
        """The host's float64 invertibility check (api.CameraSet.check_invertible) on the LIVE rows over the set's frame: reads
        the rows back, and raises ValueError naming camera and pixel.  The refinement's clamps do not guarantee this."""
        if self.image_set is None or getattr(self.image_set, "cameras", None) is None:
            raise RuntimeError("check_cameras: attach_images() with a set built with cameras= first")
        self.image_set.cameras.refresh_host().check_invertible(self.image_set.width, self.image_set.height)

    def _camera_arrays(self):
        """the intrinsics refinement's share of a checkpoint (nothing without refine_cameras): a missing key means zeros on loading"""
        if self._cams is None:
            return {}
        return {"camera_delta": self.camera_delta, "camera_m": self._cam_m, "camera_v": self._cam_v, "camera_steps": self.camera_updates,
                "camera_skipped": self.camera_skipped}

    def refined_poses(self):
        """[N, 4, 4]: the attached set's poses as the refinement has left them (a copy)"""
        if self.image_set is None:
            raise RuntimeError("refined_poses: call attach_images() first")
        return self.image_set.poses.view(-1, 4, 4).clone()

    def reset_poses(self):
        """Zero the pose correction, its moments and counts, and restore the poses as attached."""
        if self._pose is None:
            raise RuntimeError("reset_poses: attach_images(refine_poses=...) first")
        for t in self._pose_arrays().values():
            t.zero_()
        self.image_set.poses.copy_(self.poses0)

    def _pose_arrays(self):
        """the pose refinement's share of a checkpoint (nothing without refine_poses): optional on loading, a missing key means zeros"""
        if self._pose is None:
            return {}
        return {"pose_delta": self.pose_delta, "pose_m": self._pose_m, "pose_v": self._pose_v, "pose_steps": self.pose_updates,
                "pose_skipped": self.pose_skipped}

    def _pose_update(self, n, rays_d):
        """enqueue: the pose and camera gradients of the batch just stepped (its rays drawn from the attached set), then their
        steps -- both gradients see the rotation and the rows the batch was drawn with"""
        if self._pose is not None:
            api.pose_gradients(self.drawn, rays_d, self.rays_o_grad, self.rays_d_grad, n, self._pose)
        if self._cams is not None:
            api.camera_gradients(self.drawn, self.rays_d_grad, n, self.image_set.poses, self._cams)
        if self._pose is not None:
            api.pose_step(self._pose)
        if self._cams is not None:
            api.camera_step(self._cams)

    def _ray_gradients(self, P, n, jit):
        """enqueue: dL/d(ray) of the batch whose backward just ran, from its dencT, live list and segments"""
        api.hashgrid_input_gradient_segments(self.hg, self.table, self.start, self.end, P, self._stype(jit), self.dencT, self.dstart,
                                             self.dend, live_ws=self.live_ws if self.live_segments else None, jitter=jit,
                                             loss_scale=self.loss_scale, scale_device=self.loss_scale_now)
        api.ray_gradients_reduce(self.indices, self.num_stored, self.t_start, self.t_end, self.dstart, self.dend, n,
                                 self.rays_o_grad, self.rays_d_grad)

    def _draw_seed(self):
        seed = self.draw_seed
        if _world() > 1:                        # every rank draws its own rays
            seed = (seed + 0x632BE5AB * dist.get_rank()) & 0xFFFFFFFF
        return seed

    def _draw(self, n, rays_o, rays_d, targets, depth_targets=None):
        """enqueue: the next batch of the sequence into the given buffers, then the device counter + 1 (the host's is the caller's);
        depth_targets (a depth_weight trainer): the batch's depth targets right behind the draw, from the rays and the live poses"""
        api.draw_batch(self.image_set, n, self._draw_seed(), self._draw_step, rays_o, rays_d, targets, self.drawn)
        if depth_targets is not None:
            api.depth_targets(self.image_set, n, self.drawn, rays_d, depth_targets)
        self._draw_step.add_(1)

    def step_images(self, n=None):
        """step() on the next batch of n rays (default batch_rays) drawn from the attached image set; returns the loss scalar."""
        if self.image_set is None:
            raise RuntimeError("step_images: call attach_images() first")
        n = self.B if n is None else int(n)
        if n < 1 or n > self.B:
            raise ValueError(f"step_images: n = {n} outside [1, batch_rays = {self.B}]")
        self._draw(n, self.draw_rays_o, self.draw_rays_d, self.draw_targets, self.depth_targets)
        self.draw_count += 1
        loss = self.step(self.draw_rays_o[:n], self.draw_rays_d[:n], self.draw_targets[:n],
                         None if self._depth is None else self.depth_targets[:n])
        if (self._pose is not None or self._cams is not None) and self._stepped:       # behind the optimizer: the step sees the guard's skip word
            with _Stage(self, "pose"):
                self._pose_update(n, self.draw_rays_d)
        return loss

    def _target_width(self, targets, n):
        tc = int(targets.shape[-1]) if targets.dim() == 2 and targets.shape[0] >= n else -1
        if tc not in ((3, 4) if self.background is not None else (3,)):
            raise ValueError(f"Trainer: targets of shape {tuple(targets.shape)} for {n} rays: [n, 3]" +
                             (" or [n, 4] (straight RGBA)" if self.background is not None else " (RGBA targets need a background)"))
        return tc

    def _det_select(self):
        """Register this trainer's shadows (deterministic) or none.  They stay registered after the step: a direct backward call
        that follows runs deterministically into them while this trainer lives, and in default mode once it is collected."""
        api.set_deterministic(self._det_mlp, self._det_table)

    def _segments(self, rays_o, rays_d, n):
        kw = dict(grid_res=self.R, rays_o=rays_o, rays_d=rays_d, width=n, height=1, ray_begin=0, ray_count=n,
                  occupancy=self.occ, occupancy_coarse=self.coarse, occupancy_bricks=self.bricks, occupancy_super=self.super_mip, mode=api.TRACE_DDA,
                  viewing_direction=self.view_dirs, num_hits=self.num_hits, sub_rays=api.auto_sub_rays(n), sub_hits=self.sub_hits)
        with _Stage(self, "trace_count"):
            api.trace_grid(None, **kw)
        with _Stage(self, "scan"):
            api.scan_hits(self.num_hits[:n], self.indices[:n], self.total, self.scan_ws)
        with _Stage(self, "trace_write"):
            api.trace_grid(None, indices=self.indices, start_points=self.start, end_points=self.end, seg_view=self.seg_view,
                           num_stored=self.num_stored, segment_capacity=self.max_segments, **self._reg_t(), **kw)
        P = int(self.total.item())            # the reference synchronises here too (thrust::reduce, main.cu:632)
        if P > self.max_segments:
            # Rays whose segments do not fit are cut off ON THE DEVICE (num_stored < num_hits, never out of bounds) and
            # every later stage reads num_stored.  Raising here instead would leave the other ranks of a data-parallel
            # job waiting in the gradient all-reduce; the cut is counted and reported once.
            if self.truncated_steps == 0:
                import warnings
                warnings.warn(f"Trainer: batch needs {P} segments, capacity {self.max_segments}: rays truncated "
                              f"(raise max_segments); further truncations are counted in Trainer.truncated_steps")
            self.truncated_steps += 1
            P = self.max_segments
        return P

    def _stype(self, jitter=None):
        """The sampling type of a launch: with a jitter struct (training launches of a sample_jitter trainer) JITTER_WORLD."""
        if jitter is not None:
            return api.SAMPLING_JITTER_WORLD
        return api.SAMPLING_MIDPOINT_WORLD if self.mode == "nerf" else api.SAMPLING_REGULAR

    def _sample(self, n, P, jitter=None):
        """The standalone sampler (sampler/sampler.h:19-30): float[S][5] samples + t_vals."""
        with _Stage(self, "sampler"):
            api.launchSampler(self.start, self.end, self.view_dirs, self.t_vals, self.samples, n, self.R, self.num_stored,
                              self.indices, self._stype(jitter), jitter=jitter)
            if self.mode == "nerf" and self.density_scale != 1.0:
                self.t_vals[:P * api.NUM_SAMPLES_PER_SEGMENT].mul_(self.density_scale)

    def materialize_samples(self, n, jitter="last"):
        """Tests / inspection: run the standalone sampler over the current batch's segments (fills self.samples; t_vals are
        rewritten with the same values the folded path produced).  A sample_jitter trainer draws the offsets of the step its last
        gradients() ran at ("last"); jitter: an api.sample_jitter(...) of the caller's, or None for the midpoints."""
        if isinstance(jitter, str):
            jitter = self._jitter(self._jit_step)
        self._sample(n, min(int(self.total.item()), self.max_segments), jitter)

    def _forward(self, S, from_samples=False, save=True, jitter=None):
        """encoding + network->forward over the batch's S samples; save=False: outputs only (rendering; the first pass of the
        two-pass step).  jitter: the step's sample jitter -- a TRAINING forward, whatever `save` says; None: the midpoints."""
        P = S // api.NUM_SAMPLES_PER_SEGMENT
        t_scale = self.density_scale if self.mode == "nerf" else 1.0
        stype = self._stype(jitter)
        if self.lean_fused and not from_samples and save:
            with _Stage(self, "mlp_fwd"):       # sampler + encoder + forward: one kernel, t_vals beside the outputs
                self.net.train_forward_lean_segments(self.start, self.end, self.seg_view, P, stype, self.ws, self.out, self.radiance,
                                                     t_vals=self.t_vals, t_scale=t_scale, jitter=jitter)
            self._fused_batch = True
            return
        self._fused_batch = False
        with _Stage(self, "encode"):
            if self.fold_sampler and not from_samples:      # sampler + encoder in one pass over the segments; writes t_vals too
                if self.encoding == "hash":
                    self.hg.encode_segments(self.table, self.start, self.end, self.seg_view, P, stype, self.encT,
                                            self.t_vals, t_scale, jitter=jitter)
                else:
                    self.net.encode_frequency_segments(self.start, self.end, self.seg_view, P, stype, self.encT,
                                                       self.t_vals, t_scale, jitter=jitter)
            elif self.encoding == "hash":
                self.hg.encode(self.table, self.samples[:S], self.encT)
            else:
                self.net.encode_frequency(self.samples[:S], self.encT)
        with _Stage(self, "mlp_fwd"):
            if self.lean:
                self.net.train_forward_lean(self.encT, S, self.ws, self.out, self.radiance)
            elif self.recompute or not save:
                self.net.train_forward_outputs(self.encT, S, self.out, self.radiance)
            else:
                self.net.train_forward(self.encT, S, self.ws, self.out, self.radiance)

    def render_rays(self, rays_o, rays_d, radiance_fn=None, background=None):
        """Forward only.  radiance_fn(samples[S,5]) -> float[S,4] replaces the network (teacher rendering).  background: three
        floats composited as (1 - opacity) * background (rtxn_volrender_fwd_aux), None: black."""
        n = rays_o.shape[0]
        P = self._segments(rays_o, rays_d, n)
        S = P * api.NUM_SAMPLES_PER_SEGMENT
        if radiance_fn is not None or not self.fold_sampler:
            self._sample(n, P)
        if S:
            if radiance_fn is None:
                self._forward(S, save=False)
            else:
                self.radiance[:S] = radiance_fn(self.samples[:S])
        vr = api.VR_NERF if self.mode == "nerf" else api.VR_COMPAT
        if background is not None:
            api.volrender_fwd_aux(self.radiance, self.t_vals, self.num_stored, self.indices, n, api.NUM_SAMPLES_PER_SEGMENT,
                                  self.pixels[:n], mode=vr, background=background)
        else:
            api.launch_volrender_cuda(None, self.radiance, self.num_stored, self.indices, self.t_vals, n,
                                      api.NUM_SAMPLES_PER_SEGMENT, self.pixels[:n], mode=vr)
        return self.pixels[:n]

    def render_pipeline(self, width, height, focal_length, max_segments=None, weights="live", **kw):
        """A render.RenderPipeline over this trainer's LIVE model: the fast inference path (rtxn_render_frame: traversal, the fused
        frequency / hash-encode + MLP kernel, compact compositor; pipelined and ray-shardable) drawing whatever the parameters are
        at the time of each frame -- the pipeline holds the trainer's own model handle, hash table and occupancy tensors, and
        rtxn_mlp_set_params[_training] / Adam update them in place.  Compositor and sampling follow the trainer's mode ("nerf":
        midpoint samples, world-space steps x density_scale, exclusive transmittance; "compat": the reference's).  The
        frequency model renders through its fused inference kernel, whose weights a training-only update leaves stale:
        call sync_inference_weights() before rendering.  update_occupancy() refreshes the pipelines made here.
        weights="ema" (ema_decay; call sync_ema() first, and again whenever the frames should follow the training): the pipeline is
        built over the averaged model and fp16 table sync_ema() fills instead of the live ones; render_rays(), update_occupancy()
        and refresh_occupancy() stay on the live weights.  A model without a fused inference kernel renders its average from
        ema_parameters()."""
        from . import render
        nerf = self.mode == "nerf"
        if weights not in ("live", "ema"):
            raise ValueError(f"render_pipeline: weights = {weights!r}: 'live' or 'ema'")
        net, table = self.net, getattr(self, "table", None)
        if weights == "ema":
            if self._ema is None:
                raise RuntimeError("render_pipeline(weights='ema'): this trainer was made without ema_decay")
            if self._ema_net is None:
                raise RuntimeError("render_pipeline(weights='ema'): call sync_ema() first")
            net, table = self._ema_net, self._ema_table16
        if self.encoding == "hash":
            self._require_fused_inference(weights)
            kw.update(hashgrid=self.hg, table=table)
        pipe = render.RenderPipeline(net, self.R, width, height, focal_length, occupancy=self.occ, max_segments=max_segments,
                                     vr_mode=api.VR_NERF if nerf else api.VR_COMPAT, step_scale=self.density_scale if nerf else 1.0, **kw)
        self._pipelines = [r for r in getattr(self, "_pipelines", []) if r() is not None] + [weakref.ref(pipe)]
        return pipe

    def _require_fused_inference(self, weights):
        """render_pipeline's refusal of a hash model its fused inference kernel does not cover"""
        if not api.hashmlp_supported(self.net, self.hg):
            raise api._lib.RtxnError("render_pipeline: no fused hash-grid inference kernel for this model (built: 64 wide, <= 8 hidden "
                                     "layers, 2 features per level, an even number of levels); use render_rays()"
                                     + (" on a model set to ema_parameters()" if weights == "ema" else ""))

    def sync_inference_weights(self):
        """Frequency models: re-pack the fused inference kernel's weights from the current parameters (rtxn_mlp_set_params); the
        per-step update only refreshes the training layouts.  (Hash models need nothing: their one 16x16x32 packing is refreshed
        by every update.)"""
        self.net.set_params(self.params)

    def evaluate(self, image_set, images=None, weights="live", background=None, ssim=True, clamp=False, out=None):
        """Score held-out frames on the device: per frame of `images` (indices into image_set, default all of them, in that
        order) one frame rendered on the fast inference path at the set's width, height, focal length and aspect ratio, with the
        pose read where it lies in image_set.poses, and one rtxn_image_metrics call against the resident frame.  A set with
        cameras (api.ImageSet(cameras=)) renders each frame through that image's camera instead (RenderPipeline.render_camera;
        the set's focal length is not read, and the cached pipeline is keyed on the camera tensor as well).  Returns a
        float64 device tensor [n, 3] (`out`, or a new one) with rows (mse, psnr, ssim); average on the device (rec.mean(0)).
        weights "live" | "ema" (ema_decay; sync_ema() is called first); frequency models get sync_inference_weights() first.
        background: what the frames are rendered over, and what a 4-channel set's frames are composited over: None takes the
        trainer's constant background (a "random" trainer must be given one for a 4-channel set); an RGB set with no background
        renders as render() does.  ssim=False leaves NaN in column 2; clamp: the frame is clamped to [0, 1] first.
        The FIRST call for a (set geometry, weights) builds and caches the render_pipeline and sizes it with calibrate() over
        the set's poses: that reads the poses and one segment count per pose on the host, once.  Every later call only enqueues
        work -- no tensor is read on the host -- and may be captured in a torch.cuda.graph (serial frames, no parallel branches;
        pass `out`, or keep the returned tensor, as with any captured allocation).  update_occupancy() and refresh_occupancy()
        reach the cached pipelines, so the scores follow the occupancy."""
        if weights not in ("live", "ema"):
            raise ValueError(f"evaluate: weights = {weights!r}: 'live' or 'ema'")
        if weights == "ema" and self._ema is None:
            raise RuntimeError("evaluate(weights='ema'): this trainer was made without ema_decay")
        if background is None and not isinstance(self.background, str):
            background = self.background
        if background is not None:
            background = tuple(float(v) for v in background)
            if len(background) != 3:
                raise ValueError(f"evaluate: background {background!r}: three floats")
        if image_set.channels == 4 and background is None:
            raise ValueError("evaluate: a 4-channel image set needs a colour to composite its frames over: this trainer's background is "
                             + ("'random'" if self.background == "random" else "None") + ", pass background=(r, g, b)")
        idx = list(range(image_set.n_images)) if images is None else [int(i) for i in images]
        for i in idx:
            if not 0 <= i < image_set.n_images:
                raise ValueError(f"evaluate: image {i} outside [0, {image_set.n_images})")
        if out is not None and (tuple(out.shape) != (len(idx), 3) or out.dtype != torch.float64 or not out.is_contiguous()):
            raise ValueError(f"evaluate: out of shape {tuple(out.shape)} / {out.dtype}: contiguous float64 [{len(idx)}, 3]")
        if self.encoding == "hash":
            self._require_fused_inference(weights)
        else:
            self.sync_inference_weights()
        if weights == "ema":
            self.sync_ema()
        cams = getattr(image_set, "cameras", None)
        key = (image_set.width, image_set.height, image_set.focal_length, image_set.aspect_ratio, weights)
        if cams is not None:           # the camera tensor's identity: a graph captured over it keeps its address
            key += (cams.model, cams.n_cameras, cams.params.data_ptr())
        cache = self.__dict__.setdefault("_eval_pipelines", {})
        entry = cache.get(key)
        if entry is None or (entry[0].occ is None) != (self.occ is None):    # a trainer that started dense has its occupancy now
            cache.pop(key, None)
            # one slot: only serial frames are rendered here; "grow": a frame that outgrows the calibrated buffers (the occupancy
            # has filled up since) is scored truncated once, and the next eager call re-sizes the pipeline instead of raising
            pipe = self.render_pipeline(image_set.width, image_set.height, 1.0 if image_set.focal_length is None else image_set.focal_length,
                                        weights=weights, aspect_ratio=image_set.aspect_ratio, n_slots=1, on_overflow="grow")
            pipe.calibrate(image_set.poses.cpu().numpy(), cameras=cams)             # the one-time host read
            entry = cache[key] = (pipe, api.image_metrics_workspace(image_set))
        pipe, workspace = entry
        rec = out if out is not None else torch.empty((len(idx), 3), dtype=torch.float64, device=self.dev)
        for row, i in enumerate(idx):
            pose = image_set.poses[i]
            if cams is not None:           # the frame of that image's camera: rtxn_camera_rays + rtxn_render_frame_rays
                pixels = pipe.render_camera(cams, image_set.camera_of(i), pose, background=background)[0]
            elif background is not None:
                pixels = pipe.render_ex(background=background, depth=False, opacity=False, look_at=pose)[0]
            else:
                pixels = pipe.render(look_at=pose)
            api.image_metrics(image_set, i, pixels, background=background, ssim=ssim, clamp=clamp, record=rec[row], workspace=workspace)
        return rec

    def _composite_train(self, n, targets, bg):
        """The RTXN_VR_NERF training compositor over the first n rays, one launch: the entry point of the topmost struct this
        trainer has (an inactive one below it falls through in the library)."""
        batch = (self.radiance, self.t_vals, self.num_stored, self.indices, n, api.NUM_SAMPLES_PER_SEGMENT, targets)
        out = (self.pixels[:n], self.loss_grads[:n], self.loss, self.dout)
        if self._depth is not None:              # with or without a scaler, whose device word is then the loss scale
            api.volrender_depth_train(*batch, self.loss_scale if self._scaler is None else 0.0, *out, bg, self._loss, self._reg, self._scaler,
                                      self._depth)
        elif self._scaler is not None:           # the loss scale is the scaler's device word
            api.volrender_scaled_train(*batch, self._scaler, *out, bg, self._loss, self._reg)
        elif self._reg is not None:
            api.volrender_reg_train(*batch, self.loss_scale, *out, bg, self._loss, self._reg)
        elif self._loss is not None:
            api.volrender_loss_train(*batch, self.loss_scale, *out, bg, self._loss)
        elif bg is not None:
            api.volrender_l2_train_ex(*batch, self.loss_scale, *out, bg)
        else:
            api.volrender_l2_train(*batch, self.loss_scale, *out)

    def gradients(self, rays_o, rays_d, targets, depth_targets=None):
        """Everything of a step up to (not including) the optimizer: traversal ... backward.  depth_targets (a depth_weight trainer,
        which needs them): float32 [n], the rays' depth targets in world units along the ray, 0 = none.  Leaves the loss-scaled
        gradient SUMS of this batch in self.dparams (MLP, tcnn layout) and self.dtable / self.dtable_h (hash grid: fp32 for the
        densely stored levels, fp16 for the hashed ones; table_grad() assembles them) and returns the number of samples.  The
        loss is the mean over THIS batch's 3n pixel components (tcnn L2, main.cu:759)."""
        n = rays_o.shape[0]
        K = api.NUM_SAMPLES_PER_SEGMENT
        vr = api.VR_NERF if self.mode == "nerf" else api.VR_COMPAT
        bg = self._bg(self._bg_step, self._target_width(targets, n))
        if (depth_targets is None) != (self._depth is None):
            raise ValueError("Trainer: depth_targets go with depth_weight > 0: " + ("this trainer has no depth term" if self._depth is None
                             else "pass depth_targets [n] (0 = no target), or step_images() over a set with depth maps"))
        if depth_targets is not None:
            if depth_targets.dtype != torch.float32 or depth_targets.numel() != n:
                raise ValueError(f"Trainer: depth_targets of shape {tuple(depth_targets.shape)} / {depth_targets.dtype}: float32 [{n}]")
            if depth_targets.data_ptr() != self.depth_targets.data_ptr():        # step_images(): the target kernel wrote them in place
                self.depth_targets[:n].copy_(depth_targets.reshape(n))
        if self.opacity_weight > 0.0 and targets.shape[-1] != 4:
            raise ValueError(f"Trainer: opacity_weight > 0 needs [n, 4] (straight RGBA) targets, got {tuple(targets.shape)}")
        if self._bg_step is not None and self._bg_step_host != self.step_count:
            self._bg_step.fill_(self.step_count)
            self._bg_step_host = self.step_count
        jit = self._jitter(self._jit_step)
        if self._jit_step is not None and self._jit_step_host != self.step_count:
            self._jit_step.fill_(self.step_count)
            self._jit_step_host = self.step_count
        self._det_select()
        P = self._segments(rays_o, rays_d, n)
        S = P * K
        self._grads_clean = False          # the eager optimizer leaves the gradients in place (the captured one clears them)
        with _Stage(self, "zero_grads"):
            self.dparams.zero_()
            if self.encoding == "hash":
                if self.hash_fp16:
                    self.dtable[:self.hashed_lo].zero_()
                    self.dtable_h.zero_()
                else:
                    self.dtable.zero_()
        self._dp_pending = None
        if S == 0:                        # every pixel is its background: loss and pixels, no radiance to differentiate
            loss_only = self._scaler is None and self._reg is None and self._depth is None and bg is None
            if loss_only and (self._loss is None or not (self.mode == "nerf" and self.fuse_compositor)):
                self.loss.zero_()
            else:
                self._composite_train(n, targets, bg)
            if self._rays is not None:
                self.rays_o_grad[:n].zero_()
                self.rays_d_grad[:n].zero_()
            return 0
        if not self.fold_sampler:
            self._sample(n, P, jit)
        self._forward(S, save=not self.two_pass, jitter=jit)
        if self.mode == "nerf" and self.fuse_compositor:
            with _Stage(self, "composite_fwd+l2+bwd"):   # one launch: the backward's first sweep IS the forward
                self._composite_train(n, targets, bg)
        else:
            with _Stage(self, "composite_fwd"):
                api.launch_volrender_cuda(None, self.radiance, self.num_stored, self.indices, self.t_vals, n, K,
                                          self.pixels[:n], mode=vr)
            with _Stage(self, "l2_loss"):
                if self._loss is not None:
                    api.loss(self.pixels[:n], targets, self._loss, self.loss_scale, None, self.loss_grads[:n], self.loss)
                else:
                    api.l2_loss(self.pixels[:n], targets, self.loss_scale, None, self.loss_grads[:n], self.loss)
            with _Stage(self, "composite_bwd"):
                api.launch_volrender_backward_cuda(None, self.loss_grads, self.radiance, self.t_vals, self.num_stored,
                                                   self.indices, n, K, self.dout, mode=vr)
        if self.live_segments:
            with _Stage(self, "live_segments"):
                api.live_segments(self.dout, P, self.max_segments, self.live_ws)
        if self.two_pass:
            with _Stage(self, "mlp_fwd_live"):       # the activations of the segments the backward is about to visit
                self.net.train_forward_live(self.encT, S, self.ws, self.live_ws)
        with _Stage(self, "mlp_bwd+wgrad"):
            if self.lean and getattr(self, "_fused_batch", False):
                self.net.train_backward_lean_segments(self.start, self.end, self.seg_view, P, self._stype(jit), self.out, self.dout, self.ws,
                                                      self.dparams, live_ws=self.live_ws if self.live_segments else None, jitter=jit)
            elif self.lean:
                self.net.train_backward_lean(self.encT, self.out, self.dout, S, self.ws, self.dparams,
                                             live_ws=self.live_ws if self.live_segments else None)
            elif self.live_segments and self.recompute:
                self.net.train_backward_recompute_live(self.encT, self.out, self.dout, S, self.live_ws, self.dparams, self.dencT)
            elif self.live_segments:
                self.net.train_backward_live(self.encT, self.out, self.dout, S, self.ws, self.live_ws, self.dparams, self.dencT)
            elif self.recompute:
                self.net.train_backward_recompute(self.encT, self.out, self.dout, S, self.dparams, self.dencT)
            else:
                self.net.train_backward(self.encT, self.out, self.dout, S, self.ws, self.dparams, self.dencT)
        if _world() > 1:                       # the MLP gradient is complete: its all-reduce runs beside the hash scatter
            self._dp_pending = [dist.all_reduce(self.dparams, async_op=True)]
        if self.encoding == "hash":
            with _Stage(self, "hash_bwd"):
                if self.fold_sampler:
                    self.hg.backward_segments(self.start, self.end, P, self._stype(jit), self.dencT, self.dtable,
                                              self.dtable_h if self.hash_fp16 else None, live_ws=self.live_ws if self.live_segments else None,
                                              jitter=jit)
                elif self.hash_fp16:
                    self.hg.backward_mixed(self.samples[:S], self.dencT, self.dtable, self.dtable_h)
                else:
                    self.hg.backward(self.samples[:S], self.dencT, self.dtable)
        if self._rays is not None:
            with _Stage(self, "ray_grad"):
                self._ray_gradients(P, n, jit)
        return S

    def apply_gradients(self, grad_divisor=1.0):
        """optimizer->step (main.cu:787) on self.dparams / self.dtable; grad_divisor: ranks summed into them."""
        if self._opt is not None:              # the rate comes from the device kernel the other two paths launch as well
            if self._opt_step_host != self.step_count:
                self._opt_step.fill_(self.step_count)
            with _Stage(self, "adam"):
                self._apply_opt(self._opt_step, self._opt_lr, self.loss_scale * grad_divisor, grad_divisor)
            self.step_count += 1
            self._opt_step_host = self.step_count
            self._grads_clean = True           # cleared as they were consumed, skipped step or not
            return
        self.step_count += 1
        with _Stage(self, "adam"):
            api.adam_step(self.master, self.params, self.dparams, self.adam_m, self.adam_v, self.step_count, lr=self.lr,
                          loss_scale=self.loss_scale * grad_divisor)
            self.net.set_params_training(self.params)     # the Trainer only ever runs the training kernels
            if self.encoding == "hash":
                kw = dict(lr=self.lr * 10.0, eps=1e-15, loss_scale=self.loss_scale * grad_divisor)
                lo = self.hashed_lo
                if self.table_adam_sparse:
                    self._table_adam_sparse(**kw)
                elif self.hash_fp16:     # dense levels from the fp32 gradient, hashed levels straight from the fp16 one
                    if lo > 0:
                        api.adam_step(self.table_master[:lo], self.table[:lo], self.dtable[:lo], self.table_m[:lo], self.table_v[:lo],
                                      self.step_count, **kw)
                    api.adam_step_half_grads(self.table_master[lo:], self.table[lo:], self.dtable_h, self.table_m[lo:],
                                             self.table_v[lo:], self.step_count, **kw)
                else:
                    api.adam_step(self.table_master, self.table, self.dtable, self.table_m, self.table_v, self.step_count, **kw)

    def _apply_opt(self, step, rates, ls, grad_divisor=1.0):
        """The optimizer under rtxn_optimizer_options, as rtxn_train_step_opt sequences it: the gradients are complete (data
        parallel: summed), so one pass looks for Inf / NaN, the rate kernel advances the device int32 `step`, writes the factor,
        the two bias-corrected rates (`rates`: MLP, dense table) and the skip word, and the _opt Adam kernels read them.  Every
        gradient is cleared as it is consumed.  Capturable; nothing is read on the host.
        With the loss scaler, as rtxn_train_step_scaled: the statistics pass in place of the check, the scaler kernel in place of the
        rate kernel (grad_divisor is its D), and the Adam kernels that read the multiplier it leaves; `ls` is not read."""
        parts = self._table_parts()
        # one sequence for every combination: the _ema entry points with ema None are the _scaled calls, and those with scaler None
        # the _opt calls -- the same launches (rtxn_train_step_ema sequences its calls the same way)
        ema, scaler = self._ema, self._scaler
        bufs = [self.dparams] + [g for _, g in parts]
        if scaler is not None:
            api.gradient_statistics(bufs, self._opt_guard, scaler)
            api.loss_scaler_step_ema(self._opt, scaler, ema, bufs, step, rates[0:1], lr=self.lr, table_lr=self.lr * 10.0,
                                     table_effective_lr=rates[1:2], divisor=grad_divisor)
        else:
            if self.skip_nonfinite:
                api.check_gradients(bufs, self._opt_guard)
            api.optimizer_rate_ema(self._opt, ema, step, rates[0:1], lr=self.lr, table_lr=self.lr * 10.0, table_effective_lr=rates[1:2])
        kw = dict(scaler=scaler, loss_scale=ls, zero_grads=True)
        api.adam_step_ema(self.master, self.params, self.dparams, self.adam_m, self.adam_v, rates[0:1], self._opt, ema, self.ema_mlp,
                          lr=self.lr, **kw)
        self.net.set_params_training(self.params)
        cut = lambda t, sl: None if t is None else t[sl]
        for sl, g in parts:
            if not g.numel():
                continue
            if self.table_adam_sparse:
                api.adam_step_sparse_ema(self.table_master[sl], self.table[sl], g, self.table_m[sl], self.table_v[sl], self.table_steps[sl],
                                         self._opt, ema, cut(self.ema_table, sl), cut(self.ema_stamps, sl), lr=self.lr * 10.0, eps=1e-15,
                                         weight_decay=False, **kw)
            else:
                api.adam_step_ema(self.table_master[sl], self.table[sl], g, self.table_m[sl], self.table_v[sl], rates[1:2], self._opt,
                                  ema, cut(self.ema_table, sl), lr=self.lr * 10.0, eps=1e-15, weight_decay=False, **kw)

    def _table_parts(self):
        """(slice of the table, its gradient buffer): the densely stored levels from the fp32 gradient, the hashed ones from the
        fp16 one; no hash grid: none"""
        if self.encoding != "hash":
            return []
        lo = self.hashed_lo
        return [(slice(0, lo), self.dtable[:lo]), (slice(lo, None), self.dtable_h)] if self.hash_fp16 else [(slice(None), self.dtable)]

    def _table_adam_sparse(self, **kw):
        """rtxn_adam_step_sparse over the table: the densely stored levels from the fp32 gradient, the hashed ones from the fp16 one"""
        for sl, g in self._table_parts():
            if g.numel():
                api.adam_step_sparse(self.table_master[sl], self.table[sl], g, self.table_m[sl], self.table_v[sl], self.table_steps[sl], **kw)

    def table_grad(self):
        """The hash grid's gradient as ONE fp32 vector in table layout (a copy; tests and tools).  In the default mixed form
        the hashed levels' part is held in fp16 (self.dtable_h) and only self.dtable[:hashed_lo] of the fp32 buffer is live."""
        if not self.hash_fp16:
            return self.dtable.clone()
        out = self.dtable.clone()
        out[self.hashed_lo:] = self.dtable_h.float()
        return out

    def step(self, rays_o, rays_d, targets, depth_targets=None):
        """One optimisation step on a batch of rays; returns the (device) loss scalar.  depth_targets: as gradients()'.

        Data parallel (torch.distributed initialised): every rank holds B_local rays of the global batch;
        gradients are SUMMED across ranks and the mean over ranks is folded into Adam's loss_scale divisor.  EVERY rank
        takes part in the all-reduces and runs Adam in every step -- also a rank whose rays all miss the grid (its
        gradients are zero) -- so the ranks can neither deadlock nor drift apart in step count."""
        world = _world()
        S = self.gradients(rays_o, rays_d, targets, depth_targets)
        self._stepped = not (S == 0 and world == 1)
        if not self._stepped:
            return self.loss                  # nothing to learn from: no Adam step, step_count unchanged
        if world > 1:
            with _Stage(self, "allreduce"):
                # issued by gradients() behind the MLP backward; a rank without samples returned before that and joins here
                pending, self._dp_pending = (self._dp_pending or [dist.all_reduce(self.dparams, async_op=True)]), None
                if self.encoding == "hash":
                    pending.extend(self._allreduce_table_grad())
                for w in pending:
                    w.wait()
                if self.encoding == "hash" and not self.hash_fp16:
                    self._finish_table_grad()
        self.apply_gradients(float(world))
        return self.loss

    def _allreduce_table_grad(self):
        """Sum the hash-grid gradient across ranks.  What a rank's 4096/N rays touch is NOT sparse in the hashed levels
        (83 k samples x 8 corners = 664 k touches per level against 2^19 entries at N = 8), so index + value lists would be
        larger than the table; the lever is the element size.  The densely stored leading levels (hashed_lo parameters, a few
        hundred KB) are all-reduced in fp32; the hashed levels go through an fp16 staging buffer -- tiny-cuda-nn keeps that
        gradient in fp16 throughout, and the loss scale keeps it in range -- which halves the bytes on the wire
        (config 3: 2 x 7/8 x 25.2 MB per rank and step at N = 8 instead of 2 x 7/8 x 52 MB).  Returns work handles; the
        caller waits and then calls _finish_table_grad()."""
        lo = self.hashed_lo
        n = self.dtable.numel()
        pending = []
        if lo > 0:
            pending.append(dist.all_reduce(self.dtable[:lo], async_op=True))
        if n > lo and self.hash_fp16 and self.dp_sparse:
            # Round 3: with the scatter restricted to the live segments a level IS sparse (0.2 .. 25 % of its entries per
            # rank and step): per level, lists of (index, half2) where they are smaller than the level -- see dp.py
            if self._dp_table is None:
                from .dp import Half2GradExchange
                self._dp_table = Half2GradExchange(self.dtable_h, 1 << self.hg.cfg.log2_hashmap_size,
                                                   force_lists=os.environ.get("RTXN_DP_SPARSE") == "force")
            pending.extend(self._dp_table.exchange())
            return pending
        if n > lo:
            if not self.hash_fp16:      # fp32 scatter (F != 2 or switched off): stage the hashed part in fp16 for the wire
                if self.dtable_h is None:
                    self.dtable_h = torch.empty(n - lo, dtype=torch.float16, device=self.dev)
                api.convert_f32_to_f16(self.dtable[lo:], self.dtable_h)
            pending.append(dist.all_reduce(self.dtable_h, async_op=True))
        return pending

    def _finish_table_grad(self):
        """fp32 scatter only: widen the exchanged fp16 staging copy back into dtable[hashed_lo:]."""
        if self.dtable_h is not None:
            api.convert_f16_to_f32(self.dtable_h, self.dtable[self.hashed_lo:])

    def dp_bytes_per_step(self, world):
        """Bytes one rank sends (= receives) per step in a ring all-reduce of its gradients, for DESIGN.md 6."""
        f = 2.0 * (world - 1) / world
        b = f * 4 * self.dparams.numel()
        if self.encoding == "hash":
            b += f * 4 * self.hashed_lo
            last = self._dp_table.last if self._dp_table is not None else None
            if last is not None and last["world"] == world:
                b += last["bytes"]             # what the last step's exchange of the hashed levels moved (lists + dense levels)
            else:
                b += f * 2 * (self.dtable.numel() - self.hashed_lo)      # before any exchange ran: every level dense
        return b

    def time_stages(self, rays_o, rays_d, targets, steps=5):
        """Run `steps` optimisation steps with HIP events around every stage (on the stream the kernels are launched on);
        returns {stage: mean ms}.  Diagnostic: the events add launches, so the sum exceeds an untimed step slightly."""
        acc = {}
        for _ in range(steps):
            self._stage_ev = []
            self.step(rays_o, rays_d, targets)
            torch.cuda.synchronize()
            for name, e0, e1 in self._stage_ev:
                acc.setdefault(name, []).append(e0.elapsed_time(e1))
            self._stage_ev = None
        return {k: float(np.mean(v)) for k, v in acc.items()}

    # ------------------------------------------------------------------------------------------ checkpoint
    # Layout (little endian): b"RTXNCKPT", u32 version, u32 json_len, json header, then for every entry of
    # header["arrays"] its raw bytes, 64-byte aligned.  The MLP block is the reference's params_buffer
    # (main.cu:328-342): fp32 master | fp16 params (the fp16 gradient third is not persisted) plus Adam's
    # moments; the hash grid adds its table the same way.
    def state_arrays(self):
        arrs = {"mlp_master": self.master, "mlp_params": self.params, "mlp_adam_m": self.adam_m, "mlp_adam_v": self.adam_v}
        if self.encoding == "hash":
            arrs.update(table_master=self.table_master, table_params=self.table, table_adam_m=self.table_m,
                        table_adam_v=self.table_v, table_adam_steps=self.table_steps)
        return arrs

    _EMA_ARRAYS = ("ema_state", "ema_mlp", "ema_table", "ema_table_stamps")

    def _ema_header(self):
        """the weight EMA's configuration for a checkpoint header (None without ema_decay): the decay (a float32 survives JSON's
        double exactly) and the form of the table's average"""
        if self._ema is None:
            return None
        return {"decay": float(np.float32(self.ema_decay)),
                "table": None if self.ema_table is None else "lazy" if self.ema_stamps is not None else "dense"}

    def _ema_arrays(self):
        """the weight EMA's share of a checkpoint (nothing without ema_decay): optional on loading, unlike state_arrays()"""
        if self._ema is None:
            return {}
        arrs = {"ema_state": self._ema_state, "ema_mlp": self.ema_mlp}
        if self.ema_table is not None:
            arrs["ema_table"] = self.ema_table
        if self.ema_stamps is not None:
            arrs["ema_table_stamps"] = self.ema_stamps
        return arrs

    _SCALER_WORDS = (("scale", 0, True), ("multiplier", 1, True), ("good", 2, False), ("backoffs", 3, False), ("growths", 4, False),
                     ("clipped", 5, False), ("grad_norm", 6, True))

    def _scaler_header(self):
        """the scaler's state for a checkpoint header (None without a scaler); a float32 survives JSON's double exactly"""
        if self._scaler_state is None:
            return None
        w = self._scaler_state.cpu().numpy()
        return {nm: (float(w.view(np.float32)[k]) if fl else int(w[k])) for nm, k, fl in self._SCALER_WORDS}

    def _scaler_restore(self, saved):
        """the state a loaded run continues from: the file's, or (a file written without a scaler) the initial one"""
        if self._scaler_state is None:
            return
        w = api.loss_scaler_initial_state(self._scaler)
        if saved:
            for nm, k, fl in self._SCALER_WORDS:
                if nm in saved:
                    if fl:
                        w.view(np.float32)[k] = np.float32(saved[nm])
                    else:
                        w[k] = int(saved[nm])
        self._scaler_state.copy_(torch.from_numpy(w))

    def save_checkpoint(self, path):
        """The header's "draw_count" is the number of batches DRAWN (attach_images): the loaded trainer draws batch draw_count
        next.  With capture_step(prefetch=True, draw=True) one batch is drawn ahead of the step that trains on it, so a
        checkpoint saved between replays resumes one batch further on: the pending batch is skipped, none is repeated."""
        arrs = {k: v.detach().cpu().numpy() for k, v in {**self.state_arrays(), **self._ema_arrays(), **self._pose_arrays(),
                                                           **self._camera_arrays()}.items()}
        cfg = self.net.cfg
        header = {"step": self.step_count, "draw_count": self.draw_count,
                  "skipped_steps": 0 if self._opt_guard is None else int(self._opt_guard[1].item()),
                  "loss_scaler": self._scaler_header(), "weight_ema": self._ema_header(),
                  "encoding": self.encoding, "grid_res": self.R, "mode": self.mode,
                  "mlp": {f: getattr(cfg, f) for f, _ in cfg._fields_},
                  "hashgrid": None if self.hg is None else {**{f: getattr(self.hg.cfg, f) for f, _ in self.hg.cfg._fields_},
                                                            "n_dir_freqs": self.hg.n_dir_freqs},
                  "arrays": [{"name": k, "dtype": str(a.dtype), "shape": list(a.shape)} for k, a in arrs.items()]}
        blob = json.dumps(header).encode()
        with open(path, "wb") as f:
            f.write(b"RTXNCKPT" + struct.pack("<II", self._CKPT_VERSION, len(blob)) + blob)
            for a in arrs.values():
                f.write(b"\0" * ((-f.tell()) % 64))
                f.write(np.ascontiguousarray(a).tobytes())

    # version 2 (round 3's format + a guarantee): every array of state_arrays() is in the file.  Version 1 files written before
    # the table's per-entry Adam step counts existed (or with RTXN_TABLE_ADAM=dense) lack `table_adam_steps`; loading one used
    # to leave the counts at zero beside warmed moments -- every entry's bias correction restarted at t = 1, an effective table
    # learning rate of ~0.3x for thousands of steps, silently.  Now: a missing array is an error, except that a
    # version-1 file's missing step counts are filled with the file's global step (what the dense rule would have used), loudly.
    _CKPT_VERSION = 2

    def load_checkpoint(self, path):
        with open(path, "rb") as f:
            if f.read(8) != b"RTXNCKPT":
                raise ValueError(f"{path}: not an RTXN checkpoint")
            version, n = struct.unpack("<II", f.read(8))
            header = json.loads(f.read(n))
            if version not in (1, self._CKPT_VERSION) or header["encoding"] != self.encoding:
                raise ValueError(f"{path}: version {version} / encoding {header['encoding']} does not match this trainer")
            dst = self.state_arrays()
            missing = set(dst) - {ent["name"] for ent in header["arrays"]}
            # the weight EMA's arrays are optional both ways: a file without them starts the average at u = 0, a trainer without
            # the EMA reads past them.  An average kept with another decay, or in the other form of the table's average (lazy with
            # stamps under the sparse rule, dense without under RTXN_TABLE_ADAM=dense), cannot be continued -- a lazy accumulator
            # read as a dense one is stale wherever Adam did not touch it: such a file starts the average at u = 0 as well, loudly
            ema = self._ema_arrays()
            in_file = {ent["name"] for ent in header["arrays"]}
            saved = header.get("weight_ema")
            ema_in_file = bool(in_file & {"ema_state", "ema_mlp", "ema_table", "ema_table_stamps"})
            if ema and ema_in_file and (saved != self._ema_header() or set(ema) != in_file & set(self._EMA_ARRAYS)):
                import warnings
                warnings.warn(f"{path}: the checkpoint's weight EMA ({saved}) is not this trainer's ({self._ema_header()}): "
                              "the average starts over at u = 0")
                ema_in_file = False
            if ema and not ema_in_file:
                for t in ema.values():
                    t.zero_()
                ema = {}
            pose = {**self._pose_arrays(), **self._camera_arrays()}     # optional both ways, as "draw_count" is: a missing array means zeros
            for nm, t in pose.items():
                if nm not in in_file:
                    t.zero_()
            if missing == {"table_adam_steps"} and version == 1:
                import warnings
                warnings.warn(f"{path}: version-1 checkpoint without per-entry table step counts: every entry's count is set to the "
                              f"checkpoint's step ({header['step']})")
                dst["table_adam_steps"].fill_(int(header["step"]))
            elif missing:
                raise ValueError(f"{path}: checkpoint lacks {sorted(missing)}, which this trainer's state needs")
            for ent in header["arrays"]:
                f.seek((-f.tell()) % 64, 1)
                a = np.frombuffer(f.read(int(np.prod(ent["shape"])) * np.dtype(ent["dtype"]).itemsize), dtype=ent["dtype"])
                t = dst.get(ent["name"], ema.get(ent["name"], pose.get(ent["name"])))
                if t is None:
                    continue
                if list(t.shape) != ent["shape"]:
                    raise ValueError(f"{path}: {ent['name']} has shape {ent['shape']}, model needs {list(t.shape)}")
                t.copy_(torch.from_numpy(a.reshape(ent["shape"]).copy()))
        self.step_count = header["step"]
        self.draw_count = int(header.get("draw_count", 0))       # files from before device batches: the sequence starts over
        if self._draw_step is not None:
            self._draw_step.fill_(self.draw_count)
        if self._opt_guard is not None:                          # the schedule itself has no state: it continues from `step`
            self._opt_guard.zero_()
            self._opt_guard[1] = int(header.get("skipped_steps", 0))
        self._scaler_restore(header.get("loss_scaler"))
        if self._pose is not None:
            api.pose_compose(self._pose)                         # the poses are not in the file: delta against poses0 is
        if self._cams is not None:
            api.camera_compose(self._cams)                       # ... nor are the camera rows
        self.net.set_params(self.params)
        return header

    # ------------------------------------------------------------------------------------------ captured step (hipGraph)
    _LR_TABLE = 1 << 16     # beyond ~2^16 steps the bias correction is exactly 1.0f for beta2 <= 0.999

    def capture_step(self, n_rays, launch_segments=None, prefetch=False, draw=False):
        """Capture the whole optimisation step for batches of exactly `n_rays` rays as a hipGraph: traversal (count, scan,
        write) -> rtxn_train_gradients (sampler ... backward with the segment count read ON THE DEVICE) -> Adam -> weight
        re-pack, with no host round trip anywhere (the reference synchronises for the segment count, main.cu:632, and so
        does step()).  Afterwards fill graph_rays_o / graph_rays_d / graph_targets (static device buffers) and call
        step_captured().

        launch_segments: the segment count the captured launches are SIZED for (grids and the row stride of the
        feature-major workspaces); default: the trainer's max_segments.  A batch that needs more is cut off on the device
        exactly as in step() and counted in truncated_steps; blocks past the live samples exit at once, so an estimate
        ~1.5x the typical count costs nothing measurable while a 20x one costs a few empty-block dispatches per kernel.

        prefetch=True: the traversal runs ONE BATCH AHEAD, as a parallel branch of the graph.  Traversal does not depend on
        the parameters, and on a 4096-ray batch it is pure latency (the longest ray's walk, ~80 us with the chip almost
        empty), so step_captured() then traverses the batch it is given beside the gradient kernels of the batch given to
        the PREVIOUS call: the first call only traverses (returns None), every later call returns the previous batch's loss,
        and flush_captured() trains on the last batch submitted.  Two segment-buffer sets alternate.  An occupancy grid
        updated between two calls takes effect one batch later.

        draw=True (attach_images() first): the batch is drawn inside the graph -- rtxn_draw_batch is the first node, in front of
        the traversal (with prefetch: in the traversal's forked branch, into that buffer set's own rays and targets) -- and
        step_captured() needs nothing filled in.  Default False: everything as described above.

        Data parallel: gradients and optimizer are captured as two graphs with the all-reduces between them."""
        if draw and self.image_set is None:
            raise RuntimeError("capture_step(draw=True): call attach_images() first")
        if prefetch and self.ray_gradients:
            raise ValueError("capture_step(prefetch=True) with ray_gradients: the next batch's traversal would overwrite the segment "
                             "buffers the gather reads")
        if not self.fold_sampler:
            raise RuntimeError("capture_step needs the folded sampler (RTXN_TRAIN_FOLD_SAMPLER=0 is set)")
        n = int(n_rays)
        if n < 1 or n > self.B:
            raise ValueError(f"capture_step: n_rays = {n} outside [1, batch_rays = {self.B}]")
        cap = int(launch_segments) if launch_segments else self.max_segments
        cap = max(1, min(cap, self.max_segments))
        d = self.dev
        self._det_select()                      # read by the entry points as they are captured: baked into the graphs
        self.graph_rays_o = torch.zeros((n, 3), device=d)
        self.graph_rays_d = torch.zeros((n, 3), device=d)
        self.graph_rays_d[:, 2] = 1.0
        self.graph_targets = torch.zeros((n, self.target_channels), device=d)
        self.graph_depth_targets = torch.zeros(n, device=d) if self._depth is not None else None
        self._g_n, self._g_cap, self._g_prefetch, self._g_draw = n, cap, bool(prefetch), bool(draw)
        # the traversal's outputs, once per buffer set (set 0 = the trainer's own buffers)
        names = ("view_dirs", "num_hits", "indices", "num_stored", "sub_hits", "total", "start", "end", "seg_view")
        if self.t_start is not None:
            names += ("t_start", "t_end")
        set0 = {k: getattr(self, k) for k in names}
        sets = [set0]
        if prefetch:
            s1 = {k: torch.zeros_like(v) for k, v in set0.items()}
            for k in ("start", "end", "seg_view"):       # only the launch capacity is ever written
                s1[k] = torch.zeros((cap,) + tuple(set0[k].shape[1:]), device=d)
            sets.append(s1)
        for k, st in enumerate(sets):           # the regulariser reads the t_start / t_end of the set it trains on
            st["reg"] = (None if self._reg is None else self._reg if k == 0 else
                         api.train_regularizer(self.distortion_weight, st["t_start"], st["t_end"], self.distortion))
            # ... and the depth term the targets of that set's own batch, through a struct of its own
            st["depth_targets"] = None if self._depth is None else self.depth_targets if k == 0 else torch.zeros_like(self.depth_targets)
            st["depth"] = (None if self._depth is None else self._depth if k == 0 else
                           self._depth_struct(st["depth_targets"], st["t_start"], st["t_end"]))
        for st in sets:
            st["targets"] = torch.zeros((n, self.target_channels), device=d)
            st["total_host"] = torch.zeros(1, dtype=torch.int32).pin_memory()
        if draw:                                # the rays each set's draw writes and its traversal reads (set 0: graph_rays_*)
            for k, st in enumerate(sets):
                st["rays_o"] = self.graph_rays_o if k == 0 else torch.zeros_like(self.graph_rays_o)
                st["rays_d"] = self.graph_rays_d if k == 0 else self.graph_rays_d.clone()
        self._g_sets = sets
        self._g_pending = None          # prefetch: the set that holds a traversed, not yet trained batch
        self._g_next = 0
        # bias-corrected rates per step number, computed by the library's own host function (bit-identical to step());
        # the graph looks its entry up with a device-side step counter
        T = self._LR_TABLE
        tab = np.zeros((T, 2), np.float32)
        for t in range(1, T):
            tab[t, 0] = api.adam_effective_lr(self.lr, 0.9, 0.999, t)
            tab[t, 1] = api.adam_effective_lr(self.lr * 10.0, 0.9, 0.999, t)
            if t > 64 and tab[t, 0] == tab[t - 1, 0] and tab[t, 1] == tab[t - 1, 1] and tab[t - 1, 0] == tab[t - 2, 0]:
                tab[t:] = tab[t]          # converged: the rest of the table is this value
                break
        self._g_lr_table = torch.from_numpy(tab).to(d)
        self._g_step = torch.full((1,), self.step_count, dtype=torch.int64, device=d)
        # RANDOM hashes the low 32-bit word of that counter (little endian), which _captured_apply advances after the gradients
        self._g_bg = self._bg(self._g_step.view(torch.int32)[:1], self.target_channels)
        self._g_jit = self._jitter(self._g_step.view(torch.int32)[:1])       # applied by the gradient kernels, not by the traversal
        self._g_idx = torch.zeros(1, dtype=torch.int64, device=d)
        self._g_lr = torch.zeros((1, 2), device=d)
        world = _world()
        self._g_world = world
        # data parallel + hash grid: the scatter is captured as a graph of its own (rtxn_train_batch.skip_table_backward), so
        # that the MLP gradient's all-reduce can be issued between the two and run beside it
        self._g_split = world > 1 and self.encoding == "hash" and self.live_segments
        self._g_split_table = None

        # one eager pass on a side stream (kernel attributes, lazy module state), then capture
        side = torch.cuda.Stream(device=d)
        self._g_side = side
        side.wait_stream(torch.cuda.current_stream())
        state = (self.master.clone(), self.params.clone(), self.adam_m.clone(), self.adam_v.clone())
        tstate = (self.table_master.clone(), self.table.clone(), self.table_m.clone(), self.table_v.clone(),
                  self.table_steps.clone()) if self.encoding == "hash" else None
        guard = None if self._opt_guard is None else self._opt_guard.clone()
        scaler_state = None if self._scaler_state is None else self._scaler_state.clone()
        ema_state = {k: v.clone() for k, v in self._ema_arrays().items()}
        pose_state = {k: v.clone() for k, v in self._pose_arrays().items()} if draw else {}
        cam_state = {k: v.clone() for k, v in self._camera_arrays().items()} if draw else {}
        clear_grads = self._clear_grads
        with torch.cuda.stream(side):
            clear_grads()
            for k in range(len(sets)):
                self._captured_traverse(k)
            self._captured_gradients(0)
            if self._g_split:
                self._captured_table_bwd(0)
            self._captured_apply(float(world))
            self._captured_pose()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # undo the warm-up step: same parameters and step number as before capture_step()
        for dst, src in zip((self.master, self.params, self.adam_m, self.adam_v), state):
            dst.copy_(src)
        if tstate is not None:
            for dst, src in zip((self.table_master, self.table, self.table_m, self.table_v, self.table_steps), tstate):
                dst.copy_(src)
        if guard is not None:
            self._opt_guard.copy_(guard)            # a warm-up pass over non-finite inputs is not a skipped step
        if scaler_state is not None:
            self._scaler_state.copy_(scaler_state)  # ... and moves neither the scale nor its counters
        for k, v in self._ema_arrays().items():
            v.copy_(ema_state[k])                   # ... nor is it an update of the average
        if pose_state:
            for k, v in self._pose_arrays().items():
                v.copy_(pose_state[k])              # ... nor of the poses
            api.pose_compose(self._pose)
        if cam_state:
            for k, v in self._camera_arrays().items():
                v.copy_(cam_state[k])               # ... nor of the camera rows
            api.camera_compose(self._cams)
        self.net.set_params_training(self.params)
        self._g_step.fill_(self.step_count)
        self._g_step_host = self.step_count     # host mirror of the device counter (see _sync_device_step)
        if draw:
            self._draw_step.fill_(self.draw_count)      # the warm-up's draws are not batches of the sequence
        clear_grads()
        torch.cuda.synchronize()
        for st in sets:
            st["total_host"][0] = 0        # the warm-up pass is not a step

        def capture(fn):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            return g

        def forked(k_traverse, then):
            """traversal into set k_traverse on the side stream, `then` on the capturing stream, joined at the end"""
            def body():
                main = torch.cuda.current_stream()
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._captured_traverse(k_traverse)
                then()
                main.wait_stream(side)
            return body

        def train(k, with_apply):
            def body():
                self._captured_gradients(k)
                if with_apply:
                    self._captured_apply(float(world))
                    self._captured_pose()
            return body

        one = world == 1
        if not prefetch:
            def whole():
                self._captured_traverse(0)
                train(0, one)()
            self._graphs = {"step": [capture(whole)]}
        else:
            # step[k]: traverse into set k beside training on set 1-k; flush[k]: train on set k; prime: traverse into set 0
            self._graphs = {"step": [capture(forked(k, train(1 - k, one))) for k in (0, 1)],
                            "flush": [capture(train(k, one)) for k in (0, 1)],
                            "prime": [capture(lambda k=k: self._captured_traverse(k)) for k in (0, 1)]}
        if not one:
            self._graphs["apply"] = capture(lambda: self._captured_apply(float(world)))
            if self._g_split:
                self._graphs["table_bwd"] = [capture(lambda k=k: self._captured_table_bwd(k)) for k in range(len(sets))]
        return self

    # ------------------------------------------------------------------------------------------ the step as ONE C call
    def entry_args(self, n_rays, launch_segments=None, draw=False):
        """struct rtxn_train_step_args over this trainer's buffers: what a C++ host passes to rtxn_train_step (include/rtxn.h)
        -- traversal, rtxn_train_gradients, optimizer and weight re-pack of one batch in one call.  Inputs are read from
        graph_rays_o / graph_rays_d / graph_targets (created here if capture_step() has not).  The step counter the call
        advances lives on the device (entry_step).  draw=True (attach_images() first): returns (args, draw_args), draw_args the
        struct rtxn_draw_batch_args that fills those three inputs from the image set -- what the host passes to rtxn_draw_batch in
        front of rtxn_train_step, as step_entry() then does.  A depth_weight trainer reads its depth targets from
        graph_depth_targets [n_rays]; with draw=True step_entry() launches rtxn_depth_targets between the two calls instead."""
        if draw and self.image_set is None:
            raise RuntimeError("entry_args(draw=True): call attach_images() first")
        if _world() > 1:
            raise RuntimeError("entry_args: rtxn_train_step steps the optimizer inside the call; data-parallel training exchanges the "
                               "gradients between rtxn_train_gradients and the optimizer (step() / capture_step())")
        if self.encoding == "hash" and not self.table_adam_sparse:
            raise RuntimeError("entry_args: rtxn_train_step steps the table by tiny-cuda-nn's non-matrix rule (RTXN_TABLE_ADAM=dense is set)")
        n = int(n_rays)
        cap = max(1, min(int(launch_segments) if launch_segments else self.max_segments, self.max_segments))
        d = self.dev
        if getattr(self, "graph_rays_o", None) is None or self.graph_rays_o.shape[0] != n:
            self.graph_rays_o = torch.zeros((n, 3), device=d)
            self.graph_rays_d = torch.zeros((n, 3), device=d)
            self.graph_rays_d[:, 2] = 1.0
            self.graph_targets = torch.zeros((n, self.target_channels), device=d)
        if self._depth is not None and (getattr(self, "graph_depth_targets", None) is None or self.graph_depth_targets.numel() != n):
            self.graph_depth_targets = torch.zeros(n, device=d)
        self.entry_step = torch.full((1,), self.step_count, dtype=torch.int32, device=d)
        self._entry_lr = torch.zeros(1, device=d)
        hash_ = self.encoding == "hash"
        a = api._lib.TrainStepArgs()
        a.trace = api.trace_params(grid_res=self.R, rays_o=self.graph_rays_o, rays_d=self.graph_rays_d, width=n, height=1, ray_begin=0,
                                   ray_count=n, occupancy=self.occ, occupancy_coarse=self.coarse, occupancy_bricks=self.bricks,
                                   occupancy_super=self.super_mip, mode=api.TRACE_DDA, viewing_direction=self.view_dirs,
                                   num_hits=self.num_hits, sub_rays=api.auto_sub_rays(n), sub_hits=self.sub_hits)
        a.scan_workspace = self.scan_ws.data_ptr()
        a.scan_workspace_bytes = self.scan_ws.numel() * 4
        a.batch = api.train_batch(self.net, **self._batch_kw(dict(start=self.start, end=self.end, seg_view=self.seg_view,
                                                                  num_stored=self.num_stored, indices=self.indices, total=self.total,
                                                                  targets=self.graph_targets), n, cap, self._jitter(None)),
                                  target_channels=self.graph_targets.shape[1])
        # RANDOM: step NULL = the call's own counter (entry_step) before its increment
        self._entry_bg = self._bg(None, self.graph_targets.shape[1])
        self._entry_jit = self._jitter(None)        # step NULL: likewise
        o = a.opt
        o.mlp_master, o.mlp_params_fp16 = self.master.data_ptr(), self.params.data_ptr()
        o.mlp_m, o.mlp_v = self.adam_m.data_ptr(), self.adam_v.data_ptr()
        if hash_:
            o.table_master, o.table_params_fp16 = self.table_master.data_ptr(), self.table.data_ptr()
            o.table_m, o.table_v, o.table_steps = self.table_m.data_ptr(), self.table_v.data_ptr(), self.table_steps.data_ptr()
        o.step, o.effective_lr = self.entry_step.data_ptr(), self._entry_lr.data_ptr()
        o.lr, o.beta1, o.beta2, o.eps = self.lr, 0.9, 0.999, 1e-8
        o.table_lr, o.table_eps, o.loss_scale_divisor = self.lr * 10.0, 1e-15, 1.0
        self._entry_args, self._entry_cap = a, cap
        self._entry_step_host = self.step_count      # what the device counter holds now (an eager step() in between is noticed by step_entry)
        self._entry_inputs = (self.graph_rays_o.data_ptr(), self.graph_rays_d.data_ptr(), self.graph_targets.data_ptr())
        self._clear_grads()            # the call's optimizer clears what it consumes; it must start from zeros
        self._entry_draw = self._entry_depth_targets = None
        if draw:
            self._entry_draw = api.draw_batch_args(self.image_set, n, self._draw_seed(), self._draw_step, self.graph_rays_o,
                                                   self.graph_rays_d, self.graph_targets, self.drawn)
            if self._depth is not None:         # rtxn_depth_targets behind the draw: what the host passes between the two calls
                self._entry_depth_targets = api.depth_targets_args(self.image_set, n, self.drawn, self.graph_rays_d, self.depth_targets)
            return a, self._entry_draw
        return a

    def step_entry(self):
        """One optimisation step on graph_rays_o / graph_rays_d / graph_targets through rtxn_train_step (entry_args() first).
        Returns the (device) loss scalar; like step_captured() it never reads the segment count on the host."""
        self._det_select()
        if getattr(self, "_entry_args", None) is None:
            raise RuntimeError("step_entry: call entry_args() first")
        if self._entry_inputs != (self.graph_rays_o.data_ptr(), self.graph_rays_d.data_ptr(), self.graph_targets.data_ptr()):
            # capture_step() re-created the input buffers after entry_args(): the argument block still points at the old ones
            raise RuntimeError("step_entry: graph_rays_o / graph_rays_d / graph_targets were re-allocated since entry_args(); call entry_args() again")
        if not getattr(self, "_grads_clean", False):
            self._clear_grads()
        if int(self.step_count) != getattr(self, "_entry_step_host", self.step_count):
            self.entry_step.fill_(self.step_count)
        if getattr(self, "_entry_draw", None) is not None:      # the next batch of the sequence, in front of the step
            api.draw_batch_launch(self._entry_draw)
            if self._entry_depth_targets is not None:
                api.depth_targets_launch(self._entry_depth_targets)
            self._draw_step.add_(1)
            self.draw_count += 1
        elif self._depth is not None:
            self.depth_targets[:self.graph_depth_targets.numel()].copy_(self.graph_depth_targets)
        api.train_step(self._entry_args, self._entry_bg, self._entry_jit, self._loss, self._reg, self._opt, self._scaler, self._ema,
                       rays=self._rays, pose=self._pose if self._entry_draw is not None else None,
                       cameras=self._cams if self._entry_draw is not None else None, depth=self._depth)
        self._grads_clean = True       # the call's optimizer cleared every gradient it consumed
        self.step_count += 1
        self._entry_step_host = self.step_count
        return self.loss

    def _clear_grads(self):
        self.dparams.zero_()
        if self.encoding == "hash":
            self.dtable.zero_()
            if self.dtable_h is not None:
                self.dtable_h.zero_()
        self._grads_clean = True

    def _captured_traverse(self, k):
        st, n, cap = self._g_sets[k], self._g_n, self._g_cap
        if self._g_draw:                        # the batch is drawn here, straight into this set's rays and targets
            rays_o, rays_d = st["rays_o"], st["rays_d"]
            self._draw(n, rays_o, rays_d, st["targets"], st["depth_targets"])
        else:
            rays_o, rays_d = self.graph_rays_o, self.graph_rays_d
            st["targets"].copy_(self.graph_targets)
            if st["depth_targets"] is not None:
                st["depth_targets"][:n].copy_(self.graph_depth_targets)
        kw = dict(grid_res=self.R, rays_o=rays_o, rays_d=rays_d, width=n, height=1, ray_begin=0, ray_count=n,
                  occupancy=self.occ, occupancy_coarse=self.coarse, occupancy_bricks=self.bricks, occupancy_super=self.super_mip,
                  mode=api.TRACE_DDA, viewing_direction=st["view_dirs"], num_hits=st["num_hits"], sub_rays=api.auto_sub_rays(n),
                  sub_hits=st["sub_hits"])
        api.trace_grid(None, **kw)
        api.scan_hits(st["num_hits"][:n], st["indices"][:n], st["total"], self.scan_ws)
        api.trace_grid(None, indices=st["indices"], start_points=st["start"], end_points=st["end"], seg_view=st["seg_view"],
                       num_stored=st["num_stored"], segment_capacity=cap, **self._reg_t(st), **kw)
        st["total_host"].copy_(st["total"], non_blocking=True)      # 4 bytes for a later call's truncation check

    def _captured_gradients(self, k):
        st, n, cap = self._g_sets[k], self._g_n, self._g_cap
        # no fills: the captured Adam clears every gradient as it consumes it (zero_grads), capture_step() clears them once
        api.train_gradients(self.net, **self._batch_kw(st, n, cap, self._g_jit), skip_table_backward=self._g_split, background=self._g_bg,
                            jitter=self._g_jit, loss=self._loss, regularizer=st["reg"], scaler=self._scaler, rays=self._rays,
                            depth=st["depth"])

    def _batch_kw(self, st, n, cap, jitter):
        """The keywords of api.train_batch (struct rtxn_train_batch) over this trainer's buffers; st: the segments, per-ray counts
        and targets of the batch -- the trainer's own (entry_args) or one of the captured step's sets"""
        hash_ = self.encoding == "hash"
        return dict(grid=self.hg if hash_ else None, n_dir_freqs=self.hg.n_dir_freqs if hash_ else 0, table=self.table if hash_ else None,
                    start_points=st["start"], end_points=st["end"], seg_view=st["seg_view"], num_stored=st["num_stored"],
                    indices=st["indices"], total_segments=st["total"], segment_capacity=cap, n_rays=n, sample_type=self._stype(jitter),
                    t_scale=self.density_scale if self.mode == "nerf" else 1.0,
                    vr_mode=api.VR_NERF if self.mode == "nerf" else api.VR_COMPAT, targets=st["targets"], loss_scale=self.loss_scale,
                    encT=self.encT, dencT=self.dencT, workspace=self.ws, output_half=self.out, radiance=self.radiance, t_vals=self.t_vals,
                    radiance_gradients=self.dout, pixels=self.pixels, loss_gradients=self.loss_grads, loss_sum=self.loss,
                    dparams=self.dparams, dtable=self.dtable if hash_ else None,
                    dtable_hashed_half=self.dtable_h if (hash_ and self.hash_fp16) else None,
                    live_ws=self.live_ws if self.live_segments else None, workspace_lean=self.lean)

    def _captured_table_bwd(self, k):
        """the hash scatter of set k's batch over the live list the gradient graph left (its count is on the device)"""
        st = self._g_sets[k]
        self.hg.backward_segments(st["start"], st["end"], self._g_cap, self._stype(self._g_jit), self.dencT, self.dtable,
                                  self.dtable_h if self.hash_fp16 else None, live_ws=self.live_ws, jitter=self._g_jit)

    def _captured_pose(self):
        """behind the captured optimizer: the pose gradient and step of a batch the graph drew itself"""
        if (self._pose is not None or self._cams is not None) and self._g_draw:
            self._pose_update(self._g_n, self._g_sets[0]["rays_d"])

    def _captured_apply(self, grad_divisor):
        if self._opt is not None:
            # the rate kernel advances the counter's low word itself and evaluates schedule and bias correction from it: no table
            # lookup, so the schedule keeps running past _LR_TABLE steps
            self._apply_opt(self._g_step.view(torch.int32)[:1], self._g_lr[0], self.loss_scale * grad_divisor, grad_divisor)
            return
        self._g_step.add_(1)
        torch.clamp(self._g_step, max=self._LR_TABLE - 1, out=self._g_idx)
        torch.index_select(self._g_lr_table, 0, self._g_idx, out=self._g_lr)
        lr_mlp, lr_tab = self._g_lr[0, 0:1], self._g_lr[0, 1:2]
        ls = self.loss_scale * grad_divisor
        api.adam_step_captured(self.master, self.params, self.dparams, self.adam_m, self.adam_v, lr_mlp, loss_scale=ls, zero_grads=True)
        self.net.set_params_training(self.params)
        if self.encoding == "hash" and self.table_adam_sparse:
            self._table_adam_sparse(lr=self.lr * 10.0, eps=1e-15, loss_scale=ls, zero_grads=True)    # no step number: per-entry counts
        elif self.encoding == "hash":
            lo = self.hashed_lo
            if self.hash_fp16:
                if lo > 0:
                    api.adam_step_captured(self.table_master[:lo], self.table[:lo], self.dtable[:lo], self.table_m[:lo], self.table_v[:lo],
                                           lr_tab, eps=1e-15, loss_scale=ls, zero_grads=True)
                api.adam_step_captured(self.table_master[lo:], self.table[lo:], self.dtable_h, self.table_m[lo:], self.table_v[lo:],
                                       lr_tab, eps=1e-15, loss_scale=ls, zero_grads=True)
            else:
                api.adam_step_captured(self.table_master, self.table, self.dtable, self.table_m, self.table_v, lr_tab, eps=1e-15,
                                       loss_scale=ls, zero_grads=True)

    def _sync_device_step(self):
        """The captured Adam looks its bias-corrected rate up with a DEVICE step counter that only replays advance.  An eager
        step() between two captured ones, or load_checkpoint(), moves step_count on the host alone: bring the device counter
        back in line before the next replay (host mirror compared, no synchronisation)."""
        if self._g_step_host != self.step_count:
            self._g_step.fill_(self.step_count)
            self._g_step_host = self.step_count

    def _check_truncation(self, k):
        th = self._g_sets[k]["total_host"]
        need = int(th[0])                  # written by an earlier replay (a stale read only delays the report)
        if need > self._g_cap:
            if self.truncated_steps == 0:
                import warnings
                warnings.warn(f"Trainer: a captured batch needed {need} segments, the graph is sized for {self._g_cap}: rays "
                              f"truncated (capture_step(launch_segments=...)); further truncations are counted in truncated_steps")
            self.truncated_steps += 1
            th[0] = 0

    def _finish_dp(self):
        """world > 1: sum the gradients the gradient graph left, then replay the optimizer graph"""
        pending = [dist.all_reduce(self.dparams, async_op=True)]
        if self.encoding == "hash":
            if self._g_split_table is not None:          # the scatter was left out of the gradient graph: it runs now, beside
                self._graphs["table_bwd"][self._g_split_table].replay()      # the MLP gradient's all-reduce
            pending.extend(self._allreduce_table_grad())
        for w in pending:
            w.wait()
        if self.encoding == "hash" and not self.hash_fp16:
            self._finish_table_grad()
        self._graphs["apply"].replay()

    def step_captured(self):
        """Replay the captured step on graph_rays_o / graph_rays_d / graph_targets (capture_step(draw=True): on the next batch the
        graph draws itself); returns the (device) loss scalar -- with
        prefetch, of the batch submitted by the previous call (None on the first).  Unlike step() it never looks at the
        segment count on the host: a batch without any sample still runs Adam (on a zero gradient), and a truncated batch
        is noticed a call later (truncated_steps)."""
        if getattr(self, "_graphs", None) is None:
            raise RuntimeError("step_captured: call capture_step() first (also after update_occupancy() on a trainer that "
                               "was created without an occupancy grid: its graphs were dropped)")
        if not getattr(self, "_grads_clean", False):
            self._clear_grads()                       # an eager step() ran in between: its gradients are still in the buffers
        self._sync_device_step()
        if not self._g_prefetch:
            self._check_truncation(0)
            self.step_count += 1
            self._g_step_host += 1
            self.draw_count += self._g_draw
            self._graphs["step"][0].replay()
            if self._g_world > 1:
                self._g_split_table = 0 if self._g_split else None
                self._finish_dp()
            return self.loss
        k = self._g_next
        self._g_next = 1 - k
        if self._g_pending is None:                     # nothing traversed yet: this call only traverses
            self._graphs["prime"][k].replay()
            self._g_pending = k
            self.draw_count += self._g_draw
            return None
        self._check_truncation(self._g_pending)
        self.step_count += 1
        self._g_step_host += 1
        self.draw_count += self._g_draw
        self._graphs["step"][k].replay()                # traverse into set k || train on set 1-k (the pending one)
        self._g_pending = k
        if self._g_world > 1:
            self._g_split_table = 1 - k if self._g_split else None
            self._finish_dp()
        return self.loss

    def flush_captured(self):
        """prefetch only: train on the batch the last step_captured() call submitted; returns its loss (None if there is none)."""
        if not getattr(self, "_g_prefetch", False) or self._g_pending is None:
            return None
        if getattr(self, "_graphs", None) is None:
            raise RuntimeError("flush_captured: the captured graphs were dropped (update_occupancy on a dense trainer); capture_step() again")
        if not getattr(self, "_grads_clean", False):
            self._clear_grads()
        self._sync_device_step()
        k = self._g_pending
        self._check_truncation(k)
        self.step_count += 1
        self._g_step_host += 1
        self._graphs["flush"][k].replay()
        self._g_pending = None
        if self._g_world > 1:
            self._g_split_table = k if self._g_split else None
            self._finish_dp()
        return self.loss

    # ------------------------------------------------------------------------------------------ occupancy maintenance
    @torch.no_grad()
    def update_occupancy(self, threshold=0.01, chunk=1 << 20):
        """Density-driven refresh of the occupancy grid (the reference only ever builds the dense grid once,
        main.cu:393-399): evaluate sigma at every cell centre and keep cells whose optical thickness over one
        cell, sigma * density_scale * cell_size, exceeds `threshold`.  Returns the occupied fraction."""
        R = self.R
        n = R ** 3
        chunk = min(chunk, self.samples.shape[0])
        sigma = torch.empty(n, device=self.dev)
        ax = (torch.arange(R, device=self.dev, dtype=torch.float32) + 0.5) * (2.0 / R) - 1.0
        for s0 in range(0, n, chunk):
            idx = torch.arange(s0, min(s0 + chunk, n), device=self.dev)
            z, y, x = idx % R, (idx // R) % R, idx // (R * R)                  # bit index = (x*R + y)*R + z
            pts = torch.stack([ax[x], ax[y], ax[z], torch.zeros_like(ax[x]), torch.zeros_like(ax[x])], dim=1).contiguous()
            m = pts.shape[0]
            if self.encoding == "hash":
                self.hg.encode(self.table, pts, self.encT)
            else:
                self.net.encode_frequency(pts, self.encT)
            self.net.train_forward_outputs(self.encT, m, self.out, self.radiance)
            sigma[s0:s0 + m] = self.radiance[:m, 3]
        thick = sigma * (self.density_scale * 2.0 / R)
        self._set_occupancy(api.occupancy_from_density(thick, threshold, R))
        return float((thick > threshold).float().mean().item())

    @torch.no_grad()
    def refresh_occupancy(self, threshold=0.01, decay=0.95, jitter=True, threshold_mode="min_mean", runs_per_pass=None):
        """The occupancy refresh of an instant-ngp-style loop, on the device (librtxn: rtxn_occupancy_refresh):
        sigma at one point per cell -- jittered inside the cell per run of 32 z-cells and per step -- from the live model
        through the fused inference kernels, occ_density = max(occ_density * decay, sigma * density_scale * cell size), bit =
        occ_density > threshold ("absolute") or > min(threshold, mean of occ_density) ("min_mean"), and the 4^3 mip, bricks and
        16^3 mip rebuilt.  All four are rewritten IN PLACE: captured graphs stay valid, nothing is read back and nothing
        synchronises, so the call can follow every few step_captured() without stalling them (occupancy_stats() is the call
        that looks).  runs_per_pass: runs shaded per pass (default: the grid in one pass up to 65536 runs = 2 M samples, 17 MB
        of workspace).  Frequency models re-pack their inference weights first (sync_inference_weights)."""
        R = self.R
        modes = {"absolute": api.OCC_ABSOLUTE, "min_mean": api.OCC_MIN_MEAN}
        if threshold_mode not in modes:
            raise ValueError(f"refresh_occupancy: threshold_mode {threshold_mode!r} (absolute | min_mean)")
        if not api.occupancy_refresh_supported(self.net, self.hg):
            raise api._lib.RtxnError("refresh_occupancy: no fused inference kernel for this model (built: frequency models, and hash "
                                     "models 64 wide with <= 8 hidden layers, 2 features per level and an even number of levels); "
                                     "use update_occupancy(), which evaluates the cells through the training path")
        d = self.dev
        if self.occ is None:
            # a trainer that started dense has no buffers for its graphs to read: they are dropped, as by _set_occupancy
            self.occ = torch.full(((R ** 3 + 31) // 32,), -1, dtype=torch.int32, device=d)
            if R % 4 == 0:
                self.coarse = torch.full((((R // 4) ** 3 + 31) // 32,), -1, dtype=torch.int32, device=d)
                self.bricks = torch.full(((R // 4) ** 3,), -1, dtype=torch.int64, device=d)
            if R % 16 == 0:
                self.super_mip = torch.full((((R // 16) ** 3 + 31) // 32,), -1, dtype=torch.int32, device=d)
            if getattr(self, "_graphs", None) is not None:
                self._graphs = None
        runs = api.occupancy_refresh_runs(R)
        P = max(1, min(runs, int(runs_per_pass) if runs_per_pass else 1 << 16))
        if self.occ_density is None:
            self.occ_density = torch.zeros(R ** 3, device=d)
            self._occ_out = (torch.zeros(1, dtype=torch.int32, device=d), torch.zeros(1, device=d))      # occupied bits, mean
        need = api._lib.lib().rtxn_occupancy_refresh_workspace_bytes(R, P)
        if self._occ_ws is None or self._occ_ws.numel() * 4 < need:
            self._occ_ws = api.occupancy_refresh_workspace(R, P, device=d)
        if getattr(self, "_g_step", None) is not None:
            step = self._g_step.view(torch.int32)[:1]        # the captured steps' device counter (little-endian low word)
        else:
            if self._occ_step is None:
                self._occ_step = torch.zeros(1, dtype=torch.int32, device=d)
            self._occ_step.fill_(self.step_count)
            step = self._occ_step
        if self.encoding != "hash":
            self.sync_inference_weights()
        api.occupancy_refresh(self.net, grid=self.hg, table=self.table if self.encoding == "hash" else None, grid_res=R,
                              density=self.occ_density, decay=decay, thickness_scale=self.density_scale * 2.0 / R,
                              threshold=threshold, threshold_mode=modes[threshold_mode], jitter=jitter, seed=self._occ_seed,
                              step=step, occupancy=self.occ, coarse=self.coarse, bricks=self.bricks, super_mip=self.super_mip,
                              occupied=self._occ_out[0], mean=self._occ_out[1], workspace=self._occ_ws, runs_per_pass=P)
        for ref in getattr(self, "_pipelines", []):
            pipe = ref()
            if pipe is not None and pipe.occ is not None:
                pipe.set_occupancy(self.occ)     # stream-ordered behind the refresh: the renderer rebuilds its own hierarchy
        return None

    def occupancy_stats(self):
        """(occupied fraction, mean of occ_density) as the last refresh_occupancy() left them; synchronises."""
        if self._occ_out is None:
            raise RuntimeError("occupancy_stats: call refresh_occupancy() first")
        return int(self._occ_out[0].item()) / float(self.R ** 3), float(self._occ_out[1].item())

    # ------------------------------------------------------------------------------------------------ mesh extraction
    @torch.no_grad()
    def density_lattice(self, resolution=128, aabb=None, weights="live", out=None):
        """sigma * density_scale of the model at the nodes of a regular lattice (api.density_lattice): float32
        [n_x, n_y, n_z] over aabb = (lo, hi) inside the cube (default: all of it), from the live weights or, weights="ema", from
        the averaged ones (sync_ema() is called first, as by evaluate()).  Frequency models re-pack their inference weights first
        (sync_inference_weights)."""
        if weights not in ("live", "ema"):
            raise ValueError(f"density_lattice: weights = {weights!r}: 'live' or 'ema'")
        if weights == "ema" and self._ema is None:
            raise RuntimeError("density_lattice(weights='ema'): this trainer was made without ema_decay")
        if not api.occupancy_refresh_supported(self.net, self.hg):
            raise api._lib.RtxnError("extract_mesh: no fused inference kernel for this model (built: frequency models, and hash "
                                     "models 64 wide with <= 8 hidden layers, 2 features per level and an even number of levels); "
                                     "use update_occupancy(), which evaluates the cells through the training path")
        if self.encoding != "hash":
            self.sync_inference_weights()
        net, table = self.net, (self.table if self.encoding == "hash" else None)
        if weights == "ema":
            self.sync_ema()
            net, table = self._ema_net, (self._ema_table16 if self.encoding == "hash" else None)
        return api.density_lattice(net, grid=self.hg, table=table, resolution=resolution,
                                   aabb=((-1.0,) * 3, (1.0,) * 3) if aabb is None else aabb, scale=self.density_scale, out=out)

    @torch.no_grad()
    def extract_mesh(self, resolution=128, *, iso, aabb=None, weights="live", normals=True):
        """The triangle mesh of {sigma * density_scale > iso}: density_lattice() at `resolution` nodes per axis (an int or three)
        and api.isosurface() over it (marching tetrahedra on the device).  Returns (vertices float32[V, 3],
        triangles int32[T, 3], normals float32[V, 3] | None) on the device; api.write_ply() stores them.
        iso has no default: it is an extinction per unit length of the cube's coordinates, sigma * density_scale, the quantity the
        compositor integrates -- a surface at iso is where a ray loses a fraction 1 - exp(-iso * d) over a length d.
        Vertices are in the CUBE's coordinates, [-1, 1]^3, the ones start_points and the occupancy grid use: the loader's camera
        ORIGINS are divided by 10 on their way in (origin_scale 0.1, quirk Q2), so a vertex p lies at 10 p in the units of the
        poses' translations; rotations are unchanged.  Triangles wind counter-clockwise seen from outside (lower density), and
        normals point there.  Counts once, reads the two totals on the host and allocates exactly; raises the refusal of
        refresh_occupancy() for a model without a fused inference kernel."""
        box = ((-1.0,) * 3, (1.0,) * 3) if aabb is None else aabb
        lattice = self.density_lattice(resolution, box, weights)
        v, t, nrm, _ = api.isosurface(lattice, iso, box, normals=normals)
        return v, t, nrm

    def _set_occupancy(self, occ):
        """Install a new occupancy bitfield.  The four traversal inputs (fine bits, 4^3 mip, bricks, 16^3 mip) keep their
        ADDRESSES once they exist: capture_step() bakes those device pointers into the traversal nodes of its graphs, so the
        refresh copies into the buffers the graphs read instead of re-binding the attributes (a dropped tensor's memory
        goes back to the caching allocator and may be reused under a replay).  A trainer that started dense (occupancy=None)
        has no buffer for the graphs to read, so its captured graphs are dropped and capture_step() must be called again."""
        R = self.R
        new = {"occ": occ,
               "coarse": api.build_occupancy_mip(occ, R) if R % 4 == 0 else None}
        new["bricks"] = api.build_occupancy_bricks(occ, R) if R % 4 == 0 else None
        new["super_mip"] = api.build_occupancy_mip(new["coarse"], R // 4) if R % 16 == 0 else None
        rebound = False
        for name, t in new.items():
            cur = getattr(self, name)
            if cur is not None and t is not None and cur.shape == t.shape and cur.dtype == t.dtype:
                cur.copy_(t)
            else:
                setattr(self, name, t)
                rebound = rebound or (cur is not None or t is not None)
        if rebound and getattr(self, "_graphs", None) is not None:
            self._graphs = None            # pointers changed under the captured traversal: step_captured() asks for a re-capture
        for ref in getattr(self, "_pipelines", []):
            pipe = ref()
            if pipe is not None and pipe.occ is not None:
                pipe.set_occupancy(self.occ)     # the renderer keeps its own mip / brick hierarchy: rebuild it from the new bits


def camera_rays(look_at, focal, width, height, device="cuda", origin_scale=0.1):
    """Pinhole rays of optixPrograms.cu:43-82 as explicit (o, d) tensors (host-side helper for building
    training batches from several poses; the arithmetic that matters happens in rtxn_trace_grid)."""
    la = torch.as_tensor(look_at, dtype=torch.float64).reshape(4, 4)
    xs = (2 * (torch.arange(width, dtype=torch.float64) + 0.5) / width - 1) * (width / height)
    ys = 2 * (torch.arange(height, dtype=torch.float64) + 0.5) / height - 1
    v, u = torch.meshgrid(ys, xs, indexing="ij")
    dirs = torch.stack([u, v, -torch.full_like(u, focal)], dim=-1).reshape(-1, 3)
    d = dirs @ la[:3, :3].T
    d = d / d.norm(dim=1, keepdim=True)
    o = (la[:3, 3] * origin_scale).expand_as(d)
    return o.float().contiguous().to(device), d.float().contiguous().to(device)


class RayDataset:
    """Dataset of rays resident on the device: the counterpart of the reference's dataset build (main.cu:463-543: one
    traversal launch per training image, every buffer copied to the host and four mallocs per ray) and of its
    std::random_shuffle + host batch gather (:612-629).  Here the rays (origin, direction) and their ground-truth pixels
    stay in HBM as three flat tensors and a batch is an on-device random gather; traversal happens per batch inside
    Trainer.step, so nothing per-ray is ever materialised on the host."""

    def __init__(self, rays_o, rays_d, pixels):
        self.rays_o, self.rays_d, self.pixels = rays_o, rays_d, pixels
        self.n = rays_o.shape[0]

    @classmethod
    def from_images(cls, dataset, corrected_focal=True, origin_scale=0.1, device="cuda"):
        """dataset: rtx_nerf_amd.loader.ImageDataset.  corrected_focal: 1/tan(camera_angle_x/2) in image half-widths
        instead of the reference's 1/tan(0.5*focal_px) (quirk Q1); origin_scale 0.1 is the reference's origin/10 (Q2)."""
        import math
        W, H = dataset.image_width, dataset.image_height
        if corrected_focal:
            focal = 1.0 / math.tan(0.5 * dataset.camera_angle_x)
        else:
            focal = float(np.float32(1.0) / np.tan(np.float32(0.5) * np.float32(dataset.focal)))
        ro, rd = [], []
        for pose in dataset.poses:
            o, d = camera_rays(pose, focal, W, H, device=device, origin_scale=origin_scale)
            ro.append(o)
            rd.append(d)
        ch = int(dataset.image_channels) or 3             # RTXN_LOAD_RGBA datasets keep their alpha: [N, 4]
        pix = torch.from_numpy(np.ascontiguousarray(dataset.images, dtype=np.float32).reshape(-1, ch)).to(device)
        return cls(torch.cat(ro), torch.cat(rd), pix), focal

    def sample_batch(self, batch, generator=None):
        idx = torch.randint(0, self.n, (batch,), device=self.rays_o.device, generator=generator)
        return self.rays_o[idx].contiguous(), self.rays_d[idx].contiguous(), self.pixels[idx].contiguous()


def psnr(pred, target):
    mse = float(((pred - target) ** 2).mean())
    return 10.0 * np.log10(1.0 / max(mse, 1e-12))
