// One optimisation step as one call (include/rtxn.h, rtxn_train_step): host-only sequencing of the stage entry points, as
// render.hip does for a frame.  Nothing here computes; the one kernel of its own advances the device step counter and forms
// the bias-corrected learning rate of tiny-cuda-nn's Adam for the MLP (main.cu:36-46, :787) from it, so that a replayed hipGraph
// of this call needs nothing refreshed from the host.
#include "common.h"

#include <cmath>

namespace {

// t = ++*step;  *lr_eff = lr sqrt(1 - beta2^t) / (1 - beta1^t)  -- the same single-precision expression rtxn_adam_effective_lr
// evaluates on the host.  The two powers are formed in double and rounded once: the device library's powf is an ulp or two off
// glibc's, which is correctly rounded but for rare ties, so a step through this call used to leave the eager step's parameters
// by 1e-8 from the third step on; like this the rate is the host's bit for bit (beta 0.9 / 0.999, t = 1 .. 70000: all but t = 3606,
// where glibc's own powf is the one that misrounds) and the eager, captured and one-call steps stay bit-identical in
// deterministic mode (tests/test_gpu_sample_jitter.py).  sqrtf and the division are correctly rounded on both sides.
__global__ void advance_step_kernel(int* step, float lr, float beta1, float beta2, float* lr_eff) {
  const int t = *step + 1;
  *step = t;
  const float p2 = (float)pow((double)beta2, (double)t), p1 = (float)pow((double)beta1, (double)t);
  *lr_eff = lr * sqrtf(1.0f - p2) / (1.0f - p1);
}

}  // namespace

// the table parameters whose gradient is in the fp32 buffer: those before the first hashed level, or all of them
static long fp32_gradient_params(const rtxn_train_batch& b) {
  const long n = rtxn_hashgrid_n_params(b.grid);
  if (!b.dtable_hashed_half) return n;
  for (int l = 0; rtxn_hashgrid_level_offset(b.grid, l) < n; ++l)
    if (rtxn_hashgrid_level_is_hashed(b.grid, l) == 1) return rtxn_hashgrid_level_offset(b.grid, l);
  return n;
}

// optimizer->step under options (include/rtxn.h, rtxn_optimizer_options): the gradients are complete -- one pass looks for Inf / NaN
// in every buffer the optimizer is about to consume, the rate kernel advances the step, evaluates the schedule and turns the flag
// into the skip word, and the Adam kernels read rate, factor and skip word from the device.  Weight decay: the MLP only.
// scaler (rtxn_loss_scaler; rtxn_train_step_scaled): the statistics pass in place of the check, the scaler kernel in place of the
// rate kernel, and the Adam kernels that read the multiplier it leaves -- all on the one stream.
// ema (rtxn_weight_ema; rtxn_train_step_ema): the rate call advances its update count and the Adam kernels keep the average; opt
// need not have anything switched on then.
// ONE sequence for every combination: the _ema entry points with ema == NULL are the _scaled calls, and those with scaler == NULL
// the _opt calls -- the launches of a step without the EMA are the ones it always made.
static int optimizer_step_opt(const rtxn_train_step_args* a, const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler,
                              const rtxn_weight_ema* ema, rtxn_stream_t stream) {
  const rtxn_train_batch& b = a->batch;
  const rtxn_train_state& o = a->opt;
  const bool hash = b.grid != nullptr;
  const long n_mlp = rtxn_mlp_n_params(b.mlp), n = hash ? rtxn_hashgrid_n_params(b.grid) : 0, lo = hash ? fp32_gradient_params(b) : 0;
  int rc;
  const rtxn_grad_buffer bufs[3] = {{b.dparams, n_mlp, 0}, {b.dtable, lo, 0}, {b.dtable_hashed_half, n - lo, 1}};
  if (scaler) {
    rc = rtxn_gradient_statistics(bufs, 3, opt->guard, scaler, stream);
    if (rc != RTXN_OK) return rc;
    rc = rtxn_loss_scaler_step_ema(opt, scaler, ema, bufs, 3, o.step, 1, o.lr, o.table_lr, o.beta1, o.beta2, o.effective_lr, nullptr,
                                   o.loss_scale_divisor, stream);
  } else {
    if (opt->skip_nonfinite) {
      rc = rtxn_check_gradients(bufs, 3, opt->guard, stream);
      if (rc != RTXN_OK) return rc;
    }
    rc = rtxn_optimizer_rate_ema(opt, ema, o.step, 1, o.lr, o.table_lr, o.beta1, o.beta2, o.effective_lr, nullptr, stream);
  }
  if (rc != RTXN_OK) return rc;
  const float ls = b.loss_scale * o.loss_scale_divisor;
  rc = rtxn_adam_step_ema(n_mlp, o.mlp_master, o.mlp_params_fp16, b.dparams, RTXN_ADAM_ZERO_GRADS, o.mlp_m, o.mlp_v, o.effective_lr, o.lr, o.beta1,
                          o.beta2, o.eps, ls, opt, scaler, ema, ema ? ema->mlp_ema : nullptr, stream);
  if (rc != RTXN_OK) return rc;
  rc = rtxn_mlp_set_params_training(const_cast<rtxn_mlp*>(b.mlp), o.mlp_params_fp16, stream);
  if (rc != RTXN_OK) return rc;
  if (hash) {
    __half* p16 = static_cast<__half*>(o.table_params_fp16);
    const int flags = RTXN_ADAM_ZERO_GRADS | RTXN_ADAM_NO_WEIGHT_DECAY;
    float* acc = ema ? ema->table_ema : nullptr;
    unsigned* stamps = ema ? ema->table_stamps : nullptr;
    if (lo > 0) {
      rc = rtxn_adam_step_sparse_ema(lo, o.table_master, p16, b.dtable, flags, o.table_m, o.table_v, o.table_steps, o.table_lr, o.beta1, o.beta2,
                                     o.table_eps, ls, opt, scaler, ema, acc, stamps, stream);
      if (rc != RTXN_OK) return rc;
    }
    if (lo < n) {
      rc = rtxn_adam_step_sparse_ema(n - lo, o.table_master + lo, p16 + lo, b.dtable_hashed_half, flags | RTXN_ADAM_GRADS_FP16, o.table_m + lo,
                                     o.table_v + lo, o.table_steps + lo, o.table_lr, o.beta1, o.beta2, o.table_eps, ls, opt, scaler, ema,
                                     ema ? acc + lo : nullptr, ema ? stamps + lo : nullptr, stream);
      if (rc != RTXN_OK) return rc;
    }
  }
  return RTXN_OK;
}

// optimizer->step (main.cu:787): every gradient is cleared as it is consumed.  opt: under the options (optimizer_step_opt).
static int optimizer_step(const rtxn_train_step_args* a, const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler,
                          const rtxn_weight_ema* ema, rtxn_stream_t stream) {
  if (opt) return optimizer_step_opt(a, opt, scaler, ema, stream);
  const rtxn_train_batch& b = a->batch;
  const rtxn_train_state& o = a->opt;
  const bool hash = b.grid != nullptr;
  int rc;
  advance_step_kernel<<<1, 1, 0, rtxn::as_stream(stream)>>>(o.step, o.lr, o.beta1, o.beta2, o.effective_lr);
  RTXN_LAUNCH_CHECK("advance_step_kernel");
  const float ls = b.loss_scale * o.loss_scale_divisor;
  rc = rtxn_adam_step_captured(rtxn_mlp_n_params(b.mlp), o.mlp_master, o.mlp_params_fp16, b.dparams, RTXN_ADAM_ZERO_GRADS, o.mlp_m, o.mlp_v,
                               o.effective_lr, o.beta1, o.beta2, o.eps, ls, stream);
  if (rc != RTXN_OK) return rc;
  rc = rtxn_mlp_set_params_training(const_cast<rtxn_mlp*>(b.mlp), o.mlp_params_fp16, stream);
  if (rc != RTXN_OK) return rc;
  if (hash) {
    const long n = rtxn_hashgrid_n_params(b.grid), lo = fp32_gradient_params(b);
    __half* p16 = static_cast<__half*>(o.table_params_fp16);
    if (lo > 0) {
      rc = rtxn_adam_step_sparse(lo, o.table_master, p16, b.dtable, RTXN_ADAM_ZERO_GRADS, o.table_m, o.table_v, o.table_steps, o.table_lr, o.beta1,
                                 o.beta2, o.table_eps, ls, stream);
      if (rc != RTXN_OK) return rc;
    }
    if (lo < n) {
      rc = rtxn_adam_step_sparse(n - lo, o.table_master + lo, p16 + lo, b.dtable_hashed_half, RTXN_ADAM_GRADS_FP16 | RTXN_ADAM_ZERO_GRADS,
                                 o.table_m + lo, o.table_v + lo, o.table_steps + lo, o.table_lr, o.beta1, o.beta2, o.table_eps, ls, stream);
      if (rc != RTXN_OK) return rc;
    }
  }
  return RTXN_OK;
}

// ---- the one checked path of the step and gradients ladders (common.h) ----------------------------------------------

// The name rule: a rung reports under its own name while it holds a struct of its own -- _depth: depth, _cameras: cameras, _rays: rays or pose, _ema: the EMA,
// _scaled: the scaler, _opt: options (have_opt: present for the options' own check, ACTIVE from then on) -- and is the rung below
// otherwise; _reg and the rungs below it always report under their own name.
static const char* entry_name(bool step, int rung, const rtxn::TrainOptions& o, bool have_opt) {
  static const char* const kStep[] = {"rtxn_train_step", "rtxn_train_step_ex", "rtxn_train_step_jitter", "rtxn_train_step_loss", "rtxn_train_step_reg",
                                      "rtxn_train_step_opt", "rtxn_train_step_scaled", "rtxn_train_step_ema", "rtxn_train_step_rays",
                                      "rtxn_train_step_cameras", "rtxn_train_step_depth"};
  static const char* const kGradients[] = {"rtxn_train_gradients", "rtxn_train_gradients_ex", "rtxn_train_gradients_jitter", "rtxn_train_gradients_loss",
                                           "rtxn_train_gradients_reg", nullptr, "rtxn_train_gradients_scaled", nullptr, "rtxn_train_gradients_rays", nullptr,
                                           "rtxn_train_gradients_depth"};
  if (rung == rtxn::RUNG_DEPTH && !o.depth) rung = step ? rtxn::RUNG_CAMERAS : rtxn::RUNG_RAYS;
  if (rung == rtxn::RUNG_CAMERAS && !o.cameras) rung = rtxn::RUNG_RAYS;
  if (rung == rtxn::RUNG_RAYS && !o.rays && !o.pose) rung = rtxn::RUNG_EMA;
  if (rung == rtxn::RUNG_EMA && !o.ema) rung = rtxn::RUNG_SCALED;
  if (rung == rtxn::RUNG_SCALED && !o.scaler) rung = rtxn::RUNG_OPT;
  if (rung == rtxn::RUNG_OPT && !have_opt) rung = rtxn::RUNG_REG;
  return (step ? kStep : kGradients)[rung];
}

// The order: the options (under the name they are present with), then NULL arguments, the EMA's and the scaler's requirements of
// the options, then jitter, background, loss, regulariser, depth, scaler, rays, pose.  A rung checks what its signature has: the rungs
// below _jitter leave a missing jitter to rtxn_train_gradients, as they always did.
int rtxn::check_train_options(rtxn::TrainRung rung, bool step, const rtxn_train_step_args* a, const rtxn_train_batch* b, rtxn::TrainOptions* o) {
  bool opt_active = false;
  int rc = rtxn::check_optimizer_options(o->opt, entry_name(step, rung, *o, o->opt != nullptr), true, &opt_active);
  if (rc != RTXN_OK) return rc;
  const char* const who = entry_name(step, rung, *o, opt_active);
  if (step) {
    RTXN_REQUIRE(a, "%s: NULL arguments", who);
    b = &a->batch;
  }
  if (rung == rtxn::RUNG_PLAIN) return RTXN_OK;                // no struct; a NULL batch: rtxn_train_gradients' own message
  RTXN_REQUIRE(b, "%s: NULL batch", who);
  if (o->ema) {
    rc = rtxn_weight_ema_check(o->ema);
    if (rc != RTXN_OK) return rc;
    RTXN_REQUIRE(o->ema->state && o->ema->mlp_ema, "%s: ema->state = %p, ema->mlp_ema = %p", who, (void*)o->ema->state, (void*)o->ema->mlp_ema);
    RTXN_REQUIRE(!b->grid || (o->ema->table_ema && o->ema->table_stamps),
                 "%s: a hash grid needs ema->table_ema and ema->table_stamps (this call steps the table by the sparse rule)", who);
    RTXN_REQUIRE(o->opt && o->opt->lr_factor && (!o->opt->skip_nonfinite || o->opt->guard),
                 "%s: the weight EMA needs options that carry lr_factor (and guard with skip_nonfinite), with or without anything switched on", who);
  }
  if (o->scaler) {
    rc = rtxn::check_loss_scaler(o->scaler, who, true);
    if (rc != RTXN_OK) return rc;
    if (step)
      RTXN_REQUIRE(o->opt && o->opt->skip_nonfinite && o->opt->guard && o->opt->lr_factor,
                   "%s: the loss scaler needs options with skip_nonfinite, guard and lr_factor: dynamic scaling implies the non-finite guard", who);
  }
  if (rung >= rtxn::RUNG_JITTER) {
    rc = rtxn::check_sample_jitter(who, b->sample_type, o->jitter, b->vr_mode);
    if (rc != RTXN_OK) return rc;
  }
  bool bg_active = false, loss_active = false, reg_active = false;
  rc = rtxn::check_train_background(o->bg, b->vr_mode, who, &bg_active);
  if (rc != RTXN_OK) return rc;
  rc = rtxn::check_train_loss(o->loss, bg_active ? o->bg->target_channels : 3, b->vr_mode, who, &loss_active);
  if (rc != RTXN_OK) return rc;
  rc = rtxn::check_train_regularizer(o->reg, b->vr_mode, b->sample_type, who, &reg_active);
  if (rc != RTXN_OK) return rc;
  if (step && reg_active)
    RTXN_REQUIRE(a->trace.mode == RTXN_TRACE_DDA, "%s: trace.mode = %d: the regulariser's t_start / t_end are written by the "
                 "RTXN_TRACE_DDA walk only, not by RTXN_TRACE_COMPAT", who, a->trace.mode);
  bool depth_active = false;
  rc = rtxn::check_train_depth(o->depth, reg_active ? o->reg : nullptr, o->rays, b->vr_mode, b->sample_type, who, &depth_active);
  if (rc != RTXN_OK) return rc;
  if (step && depth_active)
    RTXN_REQUIRE(a->trace.mode == RTXN_TRACE_DDA, "%s: trace.mode = %d: the depth term's t_start / t_end are written by the "
                 "RTXN_TRACE_DDA walk only, not by RTXN_TRACE_COMPAT", who, a->trace.mode);
  if (o->scaler) {
    if (step)
      RTXN_REQUIRE(b->vr_mode == RTXN_VR_NERF, "%s: the loss scaler needs the RTXN_VR_NERF compositor (batch.vr_mode = %d)", who, b->vr_mode);
    else
      RTXN_REQUIRE(b->vr_mode == RTXN_VR_NERF, "%s: the loss scaler needs the RTXN_VR_NERF compositor, which reads the scale from device memory "
                   "(vr_mode = %d: the three-launch route takes it by value)", who, b->vr_mode);
  }
  if (!bg_active) o->bg = nullptr;
  if (!loss_active) o->loss = nullptr;
  if (!reg_active) o->reg = nullptr;
  if (!depth_active) o->depth = nullptr;
  if (!o->ema && !opt_active) o->opt = nullptr;                // the EMA's step goes through the rate kernel, switched on or not
  if (o->rays) {
    rc = rtxn::check_ray_gradients(who, o->rays, b, o->reg);
    if (rc != RTXN_OK) return rc;
    if (step)
      RTXN_REQUIRE(a->trace.mode == RTXN_TRACE_DDA, "%s: trace.mode = %d: the ray gradients' t_start / t_end are written by the "
                   "RTXN_TRACE_DDA walk only, not by RTXN_TRACE_COMPAT", who, a->trace.mode);
  }
  if (o->pose) {
    RTXN_REQUIRE(o->rays, "%s: pose without rays: the pose gradient is formed from the ray gradients", who);
    rc = rtxn::check_pose_refinement(o->pose, who, true);
    if (rc != RTXN_OK) return rc;
    RTXN_REQUIRE(o->pose->drawn && a->trace.rays_d, "%s: pose->drawn = %p, trace.rays_d = %p: the pose gradient reads (image, pixel) per ray "
                 "and the explicit rays", who, (const void*)o->pose->drawn, (const void*)a->trace.rays_d);
  }
  if (o->cameras) {
    RTXN_REQUIRE(o->rays, "%s: cameras without rays: the intrinsics gradient is formed from the ray gradients", who);
    rc = rtxn::check_camera_refinement(o->cameras, who, true);
    if (rc != RTXN_OK) return rc;
    RTXN_REQUIRE(o->cameras->drawn && o->cameras->poses, "%s: cameras->drawn = %p, cameras->poses = %p: the intrinsics gradient reads "
                 "(image, pixel) per ray and the set's poses", who, (const void*)o->cameras->drawn, (const void*)o->cameras->poses);
  }
  if (!step) return RTXN_OK;
  // RANDOM without a counter of its own: the optimizer's, read by the compositor before the step is advanced; a jitter without one
  // likewise, by the same rule
  if (o->bg) {
    o->own_bg = *o->bg;
    if (o->own_bg.mode == RTXN_BG_RANDOM && !o->own_bg.step) o->own_bg.step = a->opt.step;
    o->bg = &o->own_bg;
  }
  if (o->jitter) {
    o->own_jitter = *o->jitter;
    if (!o->own_jitter.step) o->own_jitter.step = a->opt.step;
    o->jitter = &o->own_jitter;
  }
  return RTXN_OK;
}

// o: CHECKED options.  reg, rays: the write pass of the traversal stores t_start / t_end into their buffers; opt (ACTIVE, or
// inactive under an EMA), scaler, ema: the optimizer's (optimizer_step); pose: its gradient and step, behind the optimizer.
static int train_step_impl(const rtxn_train_step_args* a, const rtxn::TrainOptions& o, rtxn_stream_t stream) {
  const rtxn_train_batch& b = a->batch;
  const rtxn_train_state& st = a->opt;
  RTXN_REQUIRE(b.mlp, "rtxn_train_step: batch.mlp is NULL");
  RTXN_REQUIRE(b.n_rays > 0 && (uint32_t)b.n_rays == a->trace.ray_count, "rtxn_train_step: batch.n_rays = %d, trace.ray_count = %u", b.n_rays,
               a->trace.ray_count);
  RTXN_REQUIRE(a->trace.num_hits && b.indices && b.num_stored && b.total_segments && a->scan_workspace,
               "rtxn_train_step: NULL num_hits / indices / num_stored / total_segments / scan workspace");
  RTXN_REQUIRE(b.start_points && b.end_points && b.seg_view && b.segment_capacity > 0, "rtxn_train_step: NULL segment buffers or capacity %ld",
               b.segment_capacity);
  RTXN_REQUIRE(st.mlp_master && st.mlp_params_fp16 && st.mlp_m && st.mlp_v && st.step && st.effective_lr, "rtxn_train_step: NULL optimizer state");
  RTXN_REQUIRE(st.loss_scale_divisor > 0.0f, "rtxn_train_step: loss_scale_divisor = %g", st.loss_scale_divisor);
  const bool hash = b.grid != nullptr;
  if (hash)
    RTXN_REQUIRE(st.table_master && st.table_params_fp16 && st.table_m && st.table_v && st.table_steps && b.dtable,
                 "rtxn_train_step: hash grid without table optimizer state / gradient");
  RTXN_DEVICE_OR_FAIL();

  // ---- traversal: count -> scan -> write (main.cu:506-508, 631-637; the packed layout of :646-673 written by the device) ----
  rtxn_trace_params t = a->trace;
  t.indices = nullptr;
  t.start_points = t.end_points = t.t_start = t.t_end = nullptr;
  t.seg_ray = nullptr;
  t.seg_view = nullptr;
  t.seg_first = nullptr;
  t.num_stored = nullptr;
  int rc = rtxn_trace_grid(&t, stream);
  if (rc != RTXN_OK) return rc;
  rc = rtxn_scan_hits(a->trace.num_hits, const_cast<int*>(b.indices), const_cast<int*>(b.total_segments), b.n_rays, a->scan_workspace,
                      a->scan_workspace_bytes, stream);
  if (rc != RTXN_OK) return rc;
  t.indices = b.indices;
  t.start_points = const_cast<float*>(b.start_points);
  t.end_points = const_cast<float*>(b.end_points);
  t.seg_view = const_cast<float*>(b.seg_view);
  t.num_stored = const_cast<int*>(b.num_stored);
  t.segment_capacity = b.segment_capacity;
  if (o.reg) {                                                // the regulariser's distances, written beside the segments
    t.t_start = const_cast<float*>(o.reg->t_start);
    t.t_end = const_cast<float*>(o.reg->t_end);
  }
  if (o.depth) {                                              // the depth term's likewise
    t.t_start = const_cast<float*>(o.depth->t_start);
    t.t_end = const_cast<float*>(o.depth->t_end);
  }
  if (o.rays) {                                               // ... and the ray gradients': the same buffers when both are given
    t.t_start = o.rays->t_start;
    t.t_end = o.rays->t_end;
  }
  rc = rtxn_trace_grid(&t, stream);
  if (rc != RTXN_OK) return rc;

  // ---- sampler ... backward (main.cu:703-781), segment count read on the device ----
  rc = rtxn::train_gradients(&b, o, stream);
  if (rc != RTXN_OK) return rc;

  rc = optimizer_step(a, o.opt, o.scaler, o.ema, stream);
  if (rc != RTXN_OK) return rc;
  // ---- the pose and camera gradients, then their steps, behind the optimizer: the steps see the guard's skip word, and both
  // gradients the rotation and the rows the batch was drawn with ----
  if (o.pose) {
    rc = rtxn_pose_gradients(o.pose->drawn, a->trace.rays_d, o.rays->d_origin, o.rays->d_direction, b.n_rays, o.pose, stream);
    if (rc != RTXN_OK) return rc;
  }
  if (o.cameras) {
    rc = rtxn_camera_gradients(o.cameras->drawn, o.rays->d_direction, b.n_rays, o.cameras->poses, o.cameras, stream);
    if (rc != RTXN_OK) return rc;
  }
  if (o.pose) {
    rc = rtxn_pose_step(o.pose, stream);
    if (rc != RTXN_OK) return rc;
  }
  return o.cameras ? rtxn_camera_step(o.cameras, stream) : RTXN_OK;
}

// ---- the step ladder (include/rtxn.h): every rung fills the option set its signature has and takes the one checked path; what
// is NULL or switched off runs exactly what the rung without it runs.  _ex: over a background; _jitter: the sampler's jitter;
// _loss: the loss of rtxn_train_loss; _reg: the distortion regulariser; _opt: the optimizer options (optimizer.hip); _scaled: the
// dynamic loss scale, which implies the non-finite guard; _ema: the weight EMA (the options may have nothing switched on: the
// step goes through the rate kernel all the same, which advances the EMA's update count); _rays: the ray gradients and the pose
// refinement (train.hip, pose.hip); _cameras: the intrinsics refinement (camera_refine.hip); _depth: the depth term of
// rtxn_train_depth (composite_train.hip).
static int step_entry(rtxn::TrainRung rung, const rtxn_train_step_args* a, rtxn::TrainOptions o, rtxn_stream_t stream) {
  const int rc = rtxn::check_train_options(rung, true, a, nullptr, &o);
  return rc != RTXN_OK ? rc : train_step_impl(a, o, stream);
}

extern "C" int rtxn_train_step(const rtxn_train_step_args* a, rtxn_stream_t stream) { return step_entry(rtxn::RUNG_PLAIN, a, {}, stream); }

extern "C" int rtxn_train_step_ex(const rtxn_train_step_args* a, const rtxn_train_background* bg, rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_EX, a, {bg}, stream);
}

extern "C" int rtxn_train_step_jitter(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                      rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_JITTER, a, {bg, jitter}, stream);
}

extern "C" int rtxn_train_step_loss(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                    const rtxn_train_loss* loss, rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_LOSS, a, {bg, jitter, loss}, stream);
}

extern "C" int rtxn_train_step_reg(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                   const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_REG, a, {bg, jitter, loss, reg}, stream);
}

extern "C" int rtxn_train_step_opt(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                   const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                                   rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_OPT, a, {bg, jitter, loss, reg, opt}, stream);
}

extern "C" int rtxn_train_step_scaled(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                      const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                                      const rtxn_loss_scaler* scaler, rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_SCALED, a, {bg, jitter, loss, reg, opt, scaler}, stream);
}

extern "C" int rtxn_train_step_ema(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                   const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                                   const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_EMA, a, {bg, jitter, loss, reg, opt, scaler, ema}, stream);
}

extern "C" int rtxn_train_step_rays(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                    const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                                    const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, const rtxn_ray_gradients* rays,
                                    const rtxn_pose_refinement* pose, rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_RAYS, a, {bg, jitter, loss, reg, opt, scaler, ema, rays, pose}, stream);
}

extern "C" int rtxn_train_step_cameras(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                       const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                                       const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, const rtxn_ray_gradients* rays,
                                       const rtxn_pose_refinement* pose, const rtxn_camera_refinement* cameras, rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_CAMERAS, a, {bg, jitter, loss, reg, opt, scaler, ema, rays, pose, cameras}, stream);
}

extern "C" int rtxn_train_step_depth(const rtxn_train_step_args* a, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                     const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                                     const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, const rtxn_ray_gradients* rays,
                                     const rtxn_pose_refinement* pose, const rtxn_camera_refinement* cameras, const rtxn_train_depth* depth,
                                     rtxn_stream_t stream) {
  return step_entry(rtxn::RUNG_DEPTH, a, {bg, jitter, loss, reg, opt, scaler, ema, rays, pose, cameras, depth}, stream);
}
