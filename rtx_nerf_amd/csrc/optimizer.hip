// The optimizer: all of Adam (optimizer->step of the reference's training loop, main.cu:787; tiny-cuda-nn is un-vendored and
// unpinned, numerics follow oracle/rtxn_oracle.c's orc_adam_step) ...
//   adam_dense_body, adam_sparse_body    the two walks over the parameters, each written once; the six Adam kernels of this file
//                             are thin templates over them that differ in the rule for one element
//   adam_kernel, adam_sparse_kernel      the step without options: the rate by value or from one device float
// ... the optimizer options (include/rtxn.h, rtxn_optimizer_options): a learning-rate schedule evaluated on the
// device from the step counter, decoupled weight decay and a guard that skips a step whose gradients are not finite:
//   optimizer_rate_kernel     one thread: step counter, factor(t), the bias-corrected rate(s), the guard words
//   check_gradients_kernel    Inf / NaN anywhere in up to four gradient buffers -> one flag
//   adam_opt_kernel, adam_sparse_opt_kernel    adam_kernel / adam_sparse_kernel reading the rate, the factor and the skip word
//                             from device memory; kernels of their own, so that a step without options launches none of that
// ... and the dynamic loss scale with gradient-norm clipping (rtxn_loss_scaler):
//   gradient_statistics_kernel  check_gradients_kernel's pass plus a double sum of squares per block, summed in a fixed order
//   loss_scaler_kernel          optimizer_rate_kernel's sibling, one block: reduces those sums, then the rate kernel's work and
//                             the scaler's state machine (loss_scaler_advance, shared with the host)
//   adam_opt_kernel<.., true>, adam_sparse_opt_kernel<.., true>    the _opt kernels with the factor on the raw gradient read
//                             from device memory
// ... and the exponential moving average of the weights (rtxn_weight_ema):
//   adam_ema_kernel, adam_sparse_ema_kernel    the _opt kernels that also keep the average: densely, or (sparse) lazily,
//                             catching an entry up over the updates it sat out when Adam touches it
//   ema_weights_kernel          the read-out: master, accumulator, stamps, state -> debiased fp32 / fp16; stores nothing else
//   the two rate kernels advance the EMA's update count through a nullable pointer
#include "common.h"
#include "mlp_internal.h"
#include "wave_scan_internal.h"

#include <cmath>
#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr double kPi = 3.14159265358979323846;

// factor(t) of include/rtxn.h, the one restatement host and device share: everything in double, rounded to float once.  (The
// file is built with -ffp-contract=off: no product below is fused on either side.)
__host__ __device__ inline float schedule_factor(const rtxn_lr_schedule& s, int t) {
  const double warm = s.warmup_steps > 0 ? fmin(1.0, (double)t / (double)s.warmup_steps) : 1.0;
  double dec = 1.0;
  if (s.kind != RTXN_LR_CONSTANT) {
    const int past = t > s.decay_start ? t - s.decay_start : 0;
    double x = (double)past / (double)s.decay_steps;
    if (s.staircase) x = floor(x);
    const double r = (double)s.ratio;
    dec = s.kind == RTXN_LR_EXPONENTIAL ? pow(r, x) : r + (1.0 - r) * (1.0 + cos(kPi * fmin(x, 1.0))) / 2.0;
  }
  return (float)(warm * dec);
}

// t = *step (+ 1, stored, if advance); factor(t); the rates as advance_step_kernel (trainer.hip) forms them -- powers in double,
// rounded once, sqrtf and the division correctly rounded -- with lr_t = lr factor in place of lr; then the guard: the flag the
// check kernel ORed becomes this step's skip word, is cleared for the next step and counted.  One thread: every stepping path
// launches this one kernel, so their rates are the same bits by construction.
__device__ __forceinline__ unsigned rate_update(int* step, int advance, const rtxn_lr_schedule& s, float lr, float table_lr, float beta1,
                                                float beta2, float* lr_eff, float* table_lr_eff, float* factor_out, unsigned* guard) {
  int t = *step;
  if (advance) {
    t += 1;
    *step = t;
  }
  const float factor = schedule_factor(s, t);
  *factor_out = factor;
  const float p2 = (float)pow((double)beta2, (double)t), p1 = (float)pow((double)beta1, (double)t);
  *lr_eff = (lr * factor) * sqrtf(1.0f - p2) / (1.0f - p1);
  if (table_lr_eff) *table_lr_eff = (table_lr * factor) * sqrtf(1.0f - p2) / (1.0f - p1);
  unsigned bad = 0u;
  if (guard) {
    bad = guard[0] != 0u ? 1u : 0u;
    guard[0] = 0u;
    guard[1] += bad;
    guard[2] = bad;
  }
  return bad;
}

// The weight EMA's arithmetic (include/rtxn.h, rtxn_weight_ema), the one restatement host and device share.
// correction(u) = 1 / (1 - d^u) in double, rounded once; u = 0: 1.
__host__ __device__ inline float ema_correction(float d, unsigned u) {
  return u == 0u ? 1.0f : (float)(1.0 / (1.0 - pow((double)d, (double)u)));
}
// s brought over `gap` updates during which the weight stayed w: w + d^gap (s - w), one fma and one exp2 (d^gap = 2^(gap log2 d),
// as the sparse Adam forms beta^t).  gap == 0 returns s itself: w + 1 (s - w) is not s in fp32.
__host__ __device__ inline float ema_catch_up(float s, float w, unsigned gap, float log2_d) {
  if (gap == 0u) return s;
#if defined(__HIP_DEVICE_COMPILE__)
  const float p = __builtin_amdgcn_exp2f((float)gap * log2_d);
#else
  const float p = exp2f((float)gap * log2_d);
#endif
  return fmaf(p, s - w, w);
}
// behind the rate kernel's work: an applied update counts; a skipped one, and a call that does not advance the step counter
// (it only re-evaluates the rates), leave both words as they are
__device__ __forceinline__ void ema_advance(rtxn_ema_state* st, float d, unsigned bad, int advance) {
  if (!st || bad || !advance) return;
  const unsigned u = st->updates + 1u;
  st->updates = u;
  st->correction = ema_correction(d, u);
}

// ema (may be NULL): the weight EMA's state, advanced behind everything else
__global__ void optimizer_rate_kernel(int* step, int advance, rtxn_lr_schedule s, float lr, float table_lr, float beta1, float beta2,
                                      float* lr_eff, float* table_lr_eff, float* factor_out, unsigned* guard, rtxn_ema_state* ema,
                                      float ema_decay) {
  const unsigned bad = rate_update(step, advance, s, lr, table_lr, beta1, beta2, lr_eff, table_lr_eff, factor_out, guard);
  ema_advance(ema, ema_decay, bad, advance);
}

struct GradList {
  const void* data[RTXN_MAX_GRAD_BUFFERS];
  long count[RTXN_MAX_GRAD_BUFFERS];
  int is_fp16[RTXN_MAX_GRAD_BUFFERS];
};

// exponent all ones: Inf or NaN, on the raw words (two halves per word)
__device__ __forceinline__ bool nonfinite_f32(unsigned w) { return (w & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool nonfinite_h2(unsigned w) { return (w & 0x7c00u) == 0x7c00u || (w & 0x7c000000u) == 0x7c000000u; }

// the body of a buffer: four independent 16-byte loads per lane and trip (one load in flight per lane left the kernel at half the
// HBM rate on the 25 MB table gradient), then one by one
template <typename Test>
__device__ __forceinline__ bool any_word(const uint4* __restrict__ q, long body, long gid, long stride, Test nonfinite) {
  bool bad = false;
  long k = gid;
  for (; k + 3 * stride < body; k += 4 * stride) {
    const uint4 a = q[k], b = q[k + stride], c = q[k + 2 * stride], d = q[k + 3 * stride];
    bad |= nonfinite(a.x) || nonfinite(a.y) || nonfinite(a.z) || nonfinite(a.w) || nonfinite(b.x) || nonfinite(b.y) || nonfinite(b.z) ||
           nonfinite(b.w) || nonfinite(c.x) || nonfinite(c.y) || nonfinite(c.z) || nonfinite(c.w) || nonfinite(d.x) || nonfinite(d.y) ||
           nonfinite(d.z) || nonfinite(d.w);
  }
  for (; k < body; k += stride) {
    const uint4 w = q[k];
    bad |= nonfinite(w.x) || nonfinite(w.y) || nonfinite(w.z) || nonfinite(w.w);
  }
  return bad;
}

// blockIdx.y: the buffer.  Elements in front of the first 16-byte boundary and behind the last whole 16 bytes go one by one, the
// body as uint4 per lane; a wave that saw anything issues ONE atomic OR.  No lane leaves early: the ballot is over whole waves.
__global__ __launch_bounds__(kThreads) void check_gradients_kernel(GradList L, unsigned* __restrict__ flag) {
  const int b = blockIdx.y;
  const long n = L.count[b];
  const long gid = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
  const uintptr_t base = (uintptr_t)L.data[b];
  const int esize = L.is_fp16[b] ? 2 : 4, per16 = 16 / esize;
  long head = (long)(((16u - (unsigned)(base & 15u)) & 15u) / (unsigned)esize);
  if (head > n) head = n;
  const long body = (n - head) / per16, tail = head + body * per16;
  bool bad = false;
  if (L.is_fp16[b]) {
    const unsigned short* h = reinterpret_cast<const unsigned short*>(base);
    for (long i = gid; i < head; i += stride) bad |= (h[i] & 0x7c00u) == 0x7c00u;
    bad |= any_word(reinterpret_cast<const uint4*>(h + head), body, gid, stride, nonfinite_h2);
    for (long i = tail + gid; i < n; i += stride) bad |= (h[i] & 0x7c00u) == 0x7c00u;
  } else {
    const unsigned* f = reinterpret_cast<const unsigned*>(base);
    for (long i = gid; i < head; i += stride) bad |= nonfinite_f32(f[i]);
    bad |= any_word(reinterpret_cast<const uint4*>(f + head), body, gid, stride, nonfinite_f32);
    for (long i = tail + gid; i < n; i += stride) bad |= nonfinite_f32(f[i]);
  }
  const bool any = __ballot(bad) != 0;
  if (any && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// ------------------------------------------------------------------------- Adam: two walks, six kernels
// One Adam update (tcnn "Adam": no weight decay, bias correction folded into lr_eff on the host / lr_dev).
__device__ __forceinline__ void adam_one(float g, float& mi, float& vi, float& w, float lr_eff, float beta1, float beta2, float eps) {
  mi = beta1 * mi + (1.0f - beta1) * g;
  vi = beta2 * vi + (1.0f - beta2) * g * g;
  w = w - lr_eff * mi / (sqrtf(vi) + eps);
}

// The factor on the raw gradient: 1 / loss_scale by value or (DEV, rtxn_loss_scaler) the multiplier word of the scaler's state, a
// kernel-argument pointer every lane reads at the same address: one scalar load.
template <bool DEV>
using grad_factor = std::conditional_t<DEV, const float*, float>;
__device__ __forceinline__ float factor_value(float f) { return f; }
__device__ __forceinline__ float factor_value(const float* f) { return *f; }

// What a kernel hands its walk, formed behind the skip branch: the factor on the raw gradient and the update of one element.
template <typename One>
struct AdamRule {
  float grad_factor;
  One one;
};
template <typename One>
__device__ __forceinline__ AdamRule<One> adam_rule(float grad_factor, One one) { return {grad_factor, one}; }

// The six Adam kernels below are thin __global__ templates over these two walks: every instantiation is still a kernel of its
// own, under the name it always had (tools/pmc_kernels_json.py, the fingerprints under profiles/), so a step without options,
// without the scaler or without the EMA launches code that carries nothing of them -- skip is a literal nullptr there and the
// branch folds away, acc and stamps are touched under EMA alone.  What the walks fix for all of them: the alignment predicate,
// the skip branch and what it clears, the order gradient clear -> update -> stores, and (sparse) that state is loaded only for
// quads that pass the zero test.  While the features landed the kernels were copies, so that each change left the existing
// ones' code byte for byte.  Folding the copies left none of the 40 instantiations byte-identical and moved no vector-memory,
// floating-point or branch instruction, no VGPR count and no private segment off 0 in any of them: scalar address set-up and
// register names differ, and adam_kernel / adam_sparse_kernel read the grid size once where their tail loop used to read it
// again (profiles/r18/adam_bodies_ab.txt lists both builds).
//
// The dense walk.  HBM-bound (22-28 B per parameter, +8 under EMA): four parameters per thread, 16-byte accesses; pointers that
// do not allow them send every element through the scalar tail.  ZERO: the gradient is cleared as it is consumed (the next
// step accumulates into zeros without a separate fill pass).  skip (may be NULL): this step's skip word -- set, nothing of the
// state is stored, and ZERO still clears the gradient.  rule_of_step() -> AdamRule whose one(g, m, v, w, s) updates an element;
// s is the EMA accumulator's, a dummy without EMA.
template <bool HALF_GRADS, bool ZERO, bool EMA, typename RuleOfStep>
__device__ __forceinline__ void adam_dense_body(long n, float* __restrict__ master, __half* __restrict__ params, void* __restrict__ grads_v,
                                                float* __restrict__ m, float* __restrict__ v, float* __restrict__ acc,
                                                const unsigned* __restrict__ skip, RuleOfStep rule_of_step) {
  float* gf = static_cast<float*>(grads_v);
  __half* gh = static_cast<__half*>(grads_v);
  const uintptr_t acc_bits = EMA ? (uintptr_t)acc : 0;
  const bool vec = (((uintptr_t)master | (uintptr_t)m | (uintptr_t)v | acc_bits | (uintptr_t)grads_v) & 15) == 0 && ((uintptr_t)params & 7) == 0;
  const long n4 = vec ? n / 4 : 0;
  const long first = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
  if (skip && *skip != 0u) {
    if (ZERO) {
      for (long q = first; q < n4; q += stride) {
        if (HALF_GRADS) reinterpret_cast<uint2*>(gh)[q] = make_uint2(0u, 0u);
        else reinterpret_cast<float4*>(gf)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      for (long i = 4 * n4 + first; i < n; i += stride) {
        if (HALF_GRADS) gh[i] = __float2half(0.0f); else gf[i] = 0.0f;
      }
    }
    return;
  }
  const auto rule = rule_of_step();
  const float inv_loss_scale = rule.grad_factor;
  for (long q = first; q < n4; q += stride) {
    float4 w4 = reinterpret_cast<float4*>(master)[q], m4 = reinterpret_cast<float4*>(m)[q], v4 = reinterpret_cast<float4*>(v)[q];
    float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EMA) s4 = reinterpret_cast<float4*>(acc)[q];
    float g[4];
    if (HALF_GRADS) {
      const half4v h = reinterpret_cast<const half4v*>(gh)[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = (float)h[e] * inv_loss_scale;
      if (ZERO) reinterpret_cast<uint2*>(gh)[q] = make_uint2(0u, 0u);
    } else {
      const float4 f = reinterpret_cast<const float4*>(gf)[q];
      g[0] = f.x * inv_loss_scale; g[1] = f.y * inv_loss_scale; g[2] = f.z * inv_loss_scale; g[3] = f.w * inv_loss_scale;
      if (ZERO) reinterpret_cast<float4*>(gf)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    rule.one(g[0], m4.x, v4.x, w4.x, s4.x);
    rule.one(g[1], m4.y, v4.y, w4.y, s4.y);
    rule.one(g[2], m4.z, v4.z, w4.z, s4.z);
    rule.one(g[3], m4.w, v4.w, w4.w, s4.w);
    reinterpret_cast<float4*>(master)[q] = w4;
    reinterpret_cast<float4*>(m)[q] = m4;
    reinterpret_cast<float4*>(v)[q] = v4;
    if constexpr (EMA) reinterpret_cast<float4*>(acc)[q] = s4;
    const half4v o = {(_Float16)w4.x, (_Float16)w4.y, (_Float16)w4.z, (_Float16)w4.w};
    reinterpret_cast<half4v*>(params)[q] = o;
  }
  for (long i = 4 * n4 + first; i < n; i += stride) {
    const float g = (HALF_GRADS ? __half2float(gh[i]) : gf[i]) * inv_loss_scale;
    if (ZERO) { if (HALF_GRADS) gh[i] = __float2half(0.0f); else gf[i] = 0.0f; }
    float mi = m[i], vi = v[i], w = master[i], s = 0.0f;
    if constexpr (EMA) s = acc[i];
    rule.one(g, mi, vi, w, s);
    m[i] = mi;
    v[i] = vi;
    master[i] = w;
    if constexpr (EMA) acc[i] = s;
    params[i] = __float2half(w);
  }
}

// The sparse walk: tiny-cuda-nn's Adam as it treats "non-matrix" parameters -- the hash table (optimizers/adam.h, adam_step): an
// entry whose gradient is exactly zero is SKIPPED (neither moment decays, the weight stays), and the bias correction uses the
// entry's OWN count of updates (steps), "since some parameters might see fewer steps than others".  A step's batch touches
// 0.2 .. 25 % of a hashed level, so this is also the cheap form: the gradient is read everywhere (2 or 4 B per parameter), the
// 14 B of state (+8 under EMA: acc and stamps, the lazy average) only where a quad's gradient is not all +-0.  ZERO clears what
// it consumes.  skip: as above -- set, the update counts keep their bits with the rest of the state, and ZERO clears every
// non-zero gradient word (also a NaN, which is not == 0).  rule_of_step() -> AdamRule whose one(g, m, v, w, steps, s, stamp)
// leaves an element with g == 0 alone; s and stamp are dummies without EMA.
template <bool HALF_GRADS, bool ZERO, bool EMA, typename RuleOfStep>
__device__ __forceinline__ void adam_sparse_body(long n, float* __restrict__ master, __half* __restrict__ params, void* __restrict__ grads_v,
                                                 float* __restrict__ m, float* __restrict__ v, unsigned* __restrict__ steps,
                                                 float* __restrict__ acc, unsigned* __restrict__ stamps, const unsigned* __restrict__ skip,
                                                 RuleOfStep rule_of_step) {
  float* gf = static_cast<float*>(grads_v);
  __half* gh = static_cast<__half*>(grads_v);
  const uintptr_t ema_bits = EMA ? (uintptr_t)acc | (uintptr_t)stamps : 0;
  const bool vec = (((uintptr_t)master | (uintptr_t)m | (uintptr_t)v | (uintptr_t)steps | ema_bits | (uintptr_t)grads_v) & 15) == 0 &&
                   ((uintptr_t)params & 7) == 0;
  const long n4 = vec ? n / 4 : 0;
  const long first = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
  if (skip && *skip != 0u) {
    if (ZERO) {
      for (long q = first; q < n4; q += stride) {
        if (HALF_GRADS) {
          const uint2 raw = reinterpret_cast<const uint2*>(gh)[q];
          if ((raw.x | raw.y) != 0u) reinterpret_cast<uint2*>(gh)[q] = make_uint2(0u, 0u);
        } else {
          const uint4 raw = reinterpret_cast<const uint4*>(gf)[q];
          if ((raw.x | raw.y | raw.z | raw.w) != 0u) reinterpret_cast<float4*>(gf)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      for (long i = 4 * n4 + first; i < n; i += stride) {
        if (HALF_GRADS) gh[i] = __float2half(0.0f); else gf[i] = 0.0f;
      }
    }
    return;
  }
  const auto rule = rule_of_step();
  const float inv_loss_scale = rule.grad_factor;
  for (long q = first; q < n4; q += stride) {
    float g[4];
    if (HALF_GRADS) {
      const uint2 raw = reinterpret_cast<const uint2*>(gh)[q];
      if (((raw.x | raw.y) & 0x7fff7fffu) == 0u) continue;
      const half4v h = __builtin_bit_cast(half4v, raw);
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = (float)h[e] * inv_loss_scale;
      if (ZERO) reinterpret_cast<uint2*>(gh)[q] = make_uint2(0u, 0u);
    } else {
      const float4 f = reinterpret_cast<const float4*>(gf)[q];
      if (f.x == 0.0f && f.y == 0.0f && f.z == 0.0f && f.w == 0.0f) continue;
      g[0] = f.x * inv_loss_scale; g[1] = f.y * inv_loss_scale; g[2] = f.z * inv_loss_scale; g[3] = f.w * inv_loss_scale;
      if (ZERO) reinterpret_cast<float4*>(gf)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 w4 = reinterpret_cast<float4*>(master)[q], m4 = reinterpret_cast<float4*>(m)[q], v4 = reinterpret_cast<float4*>(v)[q];
    uint4 s4 = reinterpret_cast<uint4*>(steps)[q];
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
    uint4 e4 = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (EMA) {
      a4 = reinterpret_cast<float4*>(acc)[q];
      e4 = reinterpret_cast<uint4*>(stamps)[q];
    }
    rule.one(g[0], m4.x, v4.x, w4.x, s4.x, a4.x, e4.x);
    rule.one(g[1], m4.y, v4.y, w4.y, s4.y, a4.y, e4.y);
    rule.one(g[2], m4.z, v4.z, w4.z, s4.z, a4.z, e4.z);
    rule.one(g[3], m4.w, v4.w, w4.w, s4.w, a4.w, e4.w);
    reinterpret_cast<float4*>(master)[q] = w4;
    reinterpret_cast<float4*>(m)[q] = m4;
    reinterpret_cast<float4*>(v)[q] = v4;
    reinterpret_cast<uint4*>(steps)[q] = s4;
    if constexpr (EMA) {
      reinterpret_cast<float4*>(acc)[q] = a4;
      reinterpret_cast<uint4*>(stamps)[q] = e4;
    }
    const half4v o = {(_Float16)w4.x, (_Float16)w4.y, (_Float16)w4.z, (_Float16)w4.w};
    reinterpret_cast<half4v*>(params)[q] = o;
  }
  for (long i = 4 * n4 + first; i < n; i += stride) {
    const float g = (HALF_GRADS ? __half2float(gh[i]) : gf[i]) * inv_loss_scale;
    if (g == 0.0f) continue;
    if (ZERO) { if (HALF_GRADS) gh[i] = __float2half(0.0f); else gf[i] = 0.0f; }
    float mi = m[i], vi = v[i], w = master[i], s = 0.0f;
    unsigned st = steps[i], e = 0u;
    if constexpr (EMA) {
      s = acc[i];
      e = stamps[i];
    }
    rule.one(g, mi, vi, w, st, s, e);
    m[i] = mi;
    v[i] = vi;
    master[i] = w;
    steps[i] = st;
    if constexpr (EMA) {
      acc[i] = s;
      stamps[i] = e;
    }
    params[i] = __float2half(w);
  }
}

// The sparse rule's bias-corrected rate of an entry at its own update count: beta^t = 2^(t log2 beta), one v_exp_f32 each (a
// libm powf here made the kernel slower than the dense one while the gradient is still dense, early in training).  Its relative
// error is bounded by rho_sparse(t; beta1, beta2) of tests/_adam_float64.py: the instruction's one ulp of beta^t, and the
// rounded argument's 2 u t |log2 beta| ln 2 beta^t, stand against 1 - beta^t -- u (5.5 + ...) + ulp(beta2^t) / (2 (1 - beta2^t)) +
// ulp(beta1^t) / (1 - beta1^t), largest at t = 1: 4.1e-6 at betas (0.9, 0.99), 3.1e-5 at (0.9, 0.999), 3.0e-4 at (0.9, 0.9999); below
// 1e-4 while beta2 <= 0.9996.  Measured on the MI355X against float64 (profiles/r20/adam_float64.txt): at most 5.6e-7, 3.3e-6 and
// 5.0e-5 for those pairs, at t = 2 .. 3; at t = 1 the instruction returns beta to 3e-8.  A factor that multiplies lr.
__device__ __forceinline__ float adam_sparse_rate(float lr, unsigned st, float log2_beta1, float log2_beta2) {
  const float t = (float)st;
  return lr * sqrtf(1.0f - __builtin_amdgcn_exp2f(t * log2_beta2)) / (1.0f - __builtin_amdgcn_exp2f(t * log2_beta1));
}

// lr_dev (may be NULL): the bias-corrected rate of a captured step -- it changes every replay, the graph does not
template <bool HALF_GRADS, bool ZERO>
__global__ __launch_bounds__(kThreads) void adam_kernel(long n, float* __restrict__ master, __half* __restrict__ params,
                                                        void* __restrict__ grads_v, float* __restrict__ m,
                                                        float* __restrict__ v, float lr_eff, float beta1, float beta2,
                                                        float eps, float inv_loss_scale, const float* __restrict__ lr_dev) {
  if (lr_dev) lr_eff = *lr_dev;
  adam_dense_body<HALF_GRADS, ZERO, false>(n, master, params, grads_v, m, v, nullptr, nullptr, [=] {
    return adam_rule(inv_loss_scale, [=](float g, float& mi, float& vi, float& w, float&) { adam_one(g, mi, vi, w, lr_eff, beta1, beta2, eps); });
  });
}

template <bool HALF_GRADS, bool ZERO>
__global__ __launch_bounds__(kThreads) void adam_sparse_kernel(long n, float* __restrict__ master, __half* __restrict__ params,
                                                               void* __restrict__ grads_v, float* __restrict__ m, float* __restrict__ v,
                                                               unsigned* __restrict__ steps, float lr, float beta1, float beta2,
                                                               float eps, float inv_loss_scale, float log2_beta1, float log2_beta2) {
  adam_sparse_body<HALF_GRADS, ZERO, false>(n, master, params, grads_v, m, v, steps, nullptr, nullptr, nullptr, [=] {
    return adam_rule(inv_loss_scale, [=](float g, float& mi, float& vi, float& w, unsigned& st, float&, unsigned&) {
      if (g == 0.0f) return;
      st += 1u;
      adam_one(g, mi, vi, w, adam_sparse_rate(lr, st, log2_beta1, log2_beta2), beta1, beta2, eps);
    });
  });
}

// adam_kernel under the options (rtxn_optimizer_options).  lr_dev: the bias-corrected rate; factor_dev: factor(t), for the decay
// term lr_t weight_decay w with lr_t = lr factor (no bias correction); skip: this step's skip word.  DEV: the _scaled form.
template <bool HALF_GRADS, bool ZERO, bool DEV>
__global__ __launch_bounds__(kThreads) void adam_opt_kernel(long n, float* __restrict__ master, __half* __restrict__ params,
                                                            void* __restrict__ grads_v, float* __restrict__ m, float* __restrict__ v,
                                                            const float* __restrict__ lr_dev, const float* __restrict__ factor_dev, float lr,
                                                            float weight_decay, const unsigned* __restrict__ skip, float beta1, float beta2,
                                                            float eps, grad_factor<DEV> inv_loss_scale_arg) {
  adam_dense_body<HALF_GRADS, ZERO, false>(n, master, params, grads_v, m, v, nullptr, skip, [=] {
    const float inv_loss_scale = factor_value(inv_loss_scale_arg);
    const float lr_eff = *lr_dev;
    const float decay = (lr * *factor_dev) * weight_decay;          // w -= lr_t weight_decay w
    return adam_rule(inv_loss_scale, [=](float g, float& mi, float& vi, float& w, float&) {
      adam_one(g, mi, vi, w, lr_eff, beta1, beta2, eps);
      if (decay != 0.0f) w = w - decay * w;
    });
  });
}

// adam_sparse_kernel under the options: lr_t = lr factor in the entry's own bias correction, the decay term on the entries it
// updates, and the skip word.
template <bool HALF_GRADS, bool ZERO, bool DEV>
__global__ __launch_bounds__(kThreads) void adam_sparse_opt_kernel(long n, float* __restrict__ master, __half* __restrict__ params,
                                                                   void* __restrict__ grads_v, float* __restrict__ m, float* __restrict__ v,
                                                                   unsigned* __restrict__ steps, const float* __restrict__ factor_dev, float lr,
                                                                   float weight_decay, const unsigned* __restrict__ skip, float beta1,
                                                                   float beta2, float eps, grad_factor<DEV> inv_loss_scale_arg, float log2_beta1,
                                                                   float log2_beta2) {
  adam_sparse_body<HALF_GRADS, ZERO, false>(n, master, params, grads_v, m, v, steps, nullptr, nullptr, skip, [=] {
    const float inv_loss_scale = factor_value(inv_loss_scale_arg);
    const float lr_t = lr * *factor_dev;
    const float decay = lr_t * weight_decay;
    return adam_rule(inv_loss_scale, [=](float g, float& mi, float& vi, float& w, unsigned& st, float&, unsigned&) {
      if (g == 0.0f) return;
      st += 1u;
      adam_one(g, mi, vi, w, adam_sparse_rate(lr_t, st, log2_beta1, log2_beta2), beta1, beta2, eps);
      if (decay != 0.0f) w = w - decay * w;
    });
  });
}

// adam_opt_kernel that also keeps the average of what it steps (rtxn_weight_ema), dense form: s = d s + (1 - d) w behind the
// decay term, +8 bytes per element.
template <bool HALF_GRADS, bool ZERO, bool DEV>
__global__ __launch_bounds__(kThreads) void adam_ema_kernel(long n, float* __restrict__ master, __half* __restrict__ params,
                                                            void* __restrict__ grads_v, float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ acc, const float* __restrict__ lr_dev,
                                                            const float* __restrict__ factor_dev, float lr, float weight_decay,
                                                            const unsigned* __restrict__ skip, float beta1, float beta2, float eps,
                                                            grad_factor<DEV> inv_loss_scale_arg, float d, float omd) {
  adam_dense_body<HALF_GRADS, ZERO, true>(n, master, params, grads_v, m, v, acc, skip, [=] {
    const float inv_loss_scale = factor_value(inv_loss_scale_arg);
    const float lr_eff = *lr_dev;
    const float decay = (lr * *factor_dev) * weight_decay;          // w -= lr_t weight_decay w
    return adam_rule(inv_loss_scale, [=](float g, float& mi, float& vi, float& w, float& s) {
      adam_one(g, mi, vi, w, lr_eff, beta1, beta2, eps);
      if (decay != 0.0f) w = w - decay * w;
      s = d * s + omd * w;
    });
  });
}

// adam_sparse_opt_kernel that also keeps the average, lazy form: of the quads that pass the non-zero test only the updated
// elements move -- caught up over the updates they sat out, then the EMA line, then the stamp.  ema: a kernel-argument pointer
// every lane reads at the same address, one scalar load; updates was advanced by the rate kernel, so it is the number u of this
// update.
template <bool HALF_GRADS, bool ZERO, bool DEV>
__global__ __launch_bounds__(kThreads) void adam_sparse_ema_kernel(long n, float* __restrict__ master, __half* __restrict__ params,
                                                                   void* __restrict__ grads_v, float* __restrict__ m, float* __restrict__ v,
                                                                   unsigned* __restrict__ steps, float* __restrict__ acc,
                                                                   unsigned* __restrict__ stamps, const rtxn_ema_state* __restrict__ ema,
                                                                   const float* __restrict__ factor_dev, float lr, float weight_decay,
                                                                   const unsigned* __restrict__ skip, float beta1, float beta2, float eps,
                                                                   grad_factor<DEV> inv_loss_scale_arg, float log2_beta1, float log2_beta2,
                                                                   float d, float omd, float log2_d) {
  adam_sparse_body<HALF_GRADS, ZERO, true>(n, master, params, grads_v, m, v, steps, acc, stamps, skip, [=] {
    const float inv_loss_scale = factor_value(inv_loss_scale_arg);
    const float lr_t = lr * *factor_dev;
    const float decay = lr_t * weight_decay;
    const unsigned u = ema->updates;
    return adam_rule(inv_loss_scale, [=](float g, float& mi, float& vi, float& w, unsigned& st, float& s, unsigned& e) {
      if (g == 0.0f) return;
      const float w_old = w;
      st += 1u;
      adam_one(g, mi, vi, w, adam_sparse_rate(lr_t, st, log2_beta1, log2_beta2), beta1, beta2, eps);
      if (decay != 0.0f) w = w - decay * w;
      s = ema_catch_up(s, w_old, u - 1u - e, log2_d);
      s = d * s + omd * w;
      e = u;
    });
  });
}

// ---- the host side of the Adam kernels
#define ADAM_TRY(call)                 \
  do {                                 \
    const int rc_ = (call);            \
    if (rc_ != RTXN_OK) return rc_;    \
  } while (0)

// Four elements per lane.  Dense: every quad is worked on, at most 4096 blocks.  Sparse: most quads are only looked at, at most
// 8192, and at least one, which takes the tail when n < 4.
unsigned adam_dense_grid(long n) {
  const long blocks = ((n + 3) / 4 + kThreads - 1) / kThreads;
  return (unsigned)(blocks < 4096 ? blocks : 4096);
}
unsigned adam_sparse_grid(long n) {
  const long blocks = (n / 4 + kThreads - 1) / kThreads;
  return (unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks));
}

// The argument checks the entry points share, each with its one text; an entry point asks them in the order it always has.
// with_options: the calls that also take RTXN_ADAM_NO_WEIGHT_DECAY.
int check_grad_flags(const char* who, int grad_flags, bool with_options) {
  if (with_options)
    RTXN_REQUIRE((grad_flags & ~7) == 0, "%s: grad_flags = %d (RTXN_ADAM_GRADS_FP16 | RTXN_ADAM_ZERO_GRADS | RTXN_ADAM_NO_WEIGHT_DECAY)", who, grad_flags);
  else
    RTXN_REQUIRE((grad_flags & ~3) == 0, "%s: grad_flags = %d (RTXN_ADAM_GRADS_FP16 | RTXN_ADAM_ZERO_GRADS)", who, grad_flags);
  return RTXN_OK;
}
int check_betas(const char* who, float beta1, float beta2) {
  RTXN_REQUIRE(beta1 > 0.0f && beta1 < 1.0f && beta2 > 0.0f && beta2 < 1.0f, "%s: beta1 = %g, beta2 = %g outside (0, 1)", who, (double)beta1,
               (double)beta2);
  return RTXN_OK;
}

// HALF_GRADS and ZERO of grad_flags as compile-time constants: launch(half, zero) is instantiated for the four pairs, so the
// [HALF_GRADS][ZERO] table of a kernel family is the one template-id in its launch.
template <typename Launch>
void with_grad_flags(int grad_flags, Launch launch) {
  const std::true_type yes;
  const std::false_type no;
  if (grad_flags & RTXN_ADAM_GRADS_FP16) {
    if (grad_flags & RTXN_ADAM_ZERO_GRADS) launch(yes, yes); else launch(yes, no);
  } else {
    if (grad_flags & RTXN_ADAM_ZERO_GRADS) launch(no, yes); else launch(no, no);
  }
}

float adam_lr_eff(float lr, float beta1, float beta2, int step) {
  return lr * sqrtf(1.0f - powf(beta2, (float)step)) / (1.0f - powf(beta1, (float)step));
}

// the dense step without options: the rate by value, or (lr_dev) read on the device
int adam_impl(const char* who, long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v, float lr_eff,
              const float* lr_dev, float beta1, float beta2, float eps, float loss_scale, rtxn_stream_t stream) {
  RTXN_REQUIRE(loss_scale != 0.0f, "%s: loss_scale = 0", who);
  RTXN_DEVICE_OR_FAIL();
  if (n == 0) return RTXN_OK;
  RTXN_REQUIRE(master && params_fp16 && grads && m && v, "%s: NULL buffer", who);
  with_grad_flags(grad_flags, [&](auto half, auto zero) {
    adam_kernel<half(), zero()><<<adam_dense_grid(n), kThreads, 0, rtxn::as_stream(stream)>>>(
        n, master, static_cast<__half*>(params_fp16), grads, m, v, lr_eff, beta1, beta2, eps, 1.0f / loss_scale, lr_dev);
  });
  RTXN_LAUNCH_CHECK("adam_kernel");
  return RTXN_OK;
}

// Every dense step under the options, behind its entry point's checks of the structs and the flags: _opt (scaler and ema NULL),
// _scaled (ema NULL, loss_scale unused) and _ema.  The factor on the raw gradient is the scaler's multiplier word or
// 1 / loss_scale; with ema the kernel also keeps the average in ema_acc.
int adam_dense_options(const char* who, long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                       const float* effective_lr, float lr, float beta1, float beta2, float eps, float loss_scale,
                       const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, float* ema_acc,
                       rtxn_stream_t stream) {
  RTXN_REQUIRE(n >= 0 && effective_lr, "%s: n = %ld, effective_lr = %p", who, n, (const void*)effective_lr);
  RTXN_REQUIRE(scaler || loss_scale != 0.0f, "%s: loss_scale = 0", who);
  RTXN_DEVICE_OR_FAIL();
  if (n == 0) return RTXN_OK;
  RTXN_REQUIRE(master && params_fp16 && grads && m && v && (!ema || ema_acc), "%s: NULL buffer", who);
  const unsigned grid = adam_dense_grid(n);
  hipStream_t hs = rtxn::as_stream(stream);
  __half* p16 = static_cast<__half*>(params_fp16);
  const float wd = (grad_flags & RTXN_ADAM_NO_WEIGHT_DECAY) ? 0.0f : opt->weight_decay;
  const unsigned* skip = opt->skip_nonfinite ? opt->guard + 2 : nullptr;
  const float d = ema ? ema->decay : 0.0f, omd = 1.0f - d;
  auto launch = [&](auto half, auto zero, auto factor) {
    constexpr bool DEV = std::is_pointer_v<decltype(factor)>;
    if (ema)
      adam_ema_kernel<half(), zero(), DEV><<<grid, kThreads, 0, hs>>>(n, master, p16, grads, m, v, ema_acc, effective_lr, opt->lr_factor, lr, wd, skip,
                                                                      beta1, beta2, eps, factor, d, omd);
    else
      adam_opt_kernel<half(), zero(), DEV><<<grid, kThreads, 0, hs>>>(n, master, p16, grads, m, v, effective_lr, opt->lr_factor, lr, wd, skip, beta1,
                                                                      beta2, eps, factor);
  };
  with_grad_flags(grad_flags, [&](auto half, auto zero) {
    if (scaler) launch(half, zero, static_cast<const float*>(&scaler->state->multiplier)); else launch(half, zero, 1.0f / loss_scale);
  });
  RTXN_LAUNCH_CHECK(ema ? "adam_ema_kernel" : scaler ? "adam_opt_kernel (device multiplier)" : "adam_opt_kernel");
  return RTXN_OK;
}

// ... and every sparse one: _sparse_opt, _sparse_scaled and _sparse_ema, which keeps the average lazily in ema_acc and ema_stamps.
int adam_sparse_options(const char* who, long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                        unsigned* param_steps, float lr, float beta1, float beta2, float eps, float loss_scale,
                        const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, float* ema_acc,
                        unsigned* ema_stamps, rtxn_stream_t stream) {
  RTXN_REQUIRE(n >= 0, "%s: n = %ld", who, n);
  RTXN_REQUIRE(scaler || loss_scale != 0.0f, "%s: loss_scale = 0", who);
  ADAM_TRY(check_betas(who, beta1, beta2));
  RTXN_DEVICE_OR_FAIL();
  if (n == 0) return RTXN_OK;
  RTXN_REQUIRE(master && params_fp16 && grads && m && v && param_steps && (!ema || (ema_acc && ema_stamps)),
               ema ? "%s: NULL buffer (the sparse rule keeps the average lazily: ema_acc and ema_stamps)" : "%s: NULL buffer", who);
  const unsigned grid = adam_sparse_grid(n);
  hipStream_t hs = rtxn::as_stream(stream);
  __half* p16 = static_cast<__half*>(params_fp16);
  const float l2b1 = (float)log2((double)beta1), l2b2 = (float)log2((double)beta2);
  const float wd = (grad_flags & RTXN_ADAM_NO_WEIGHT_DECAY) ? 0.0f : opt->weight_decay;
  const unsigned* skip = opt->skip_nonfinite ? opt->guard + 2 : nullptr;
  const float d = ema ? ema->decay : 0.0f, omd = 1.0f - d, l2d = ema ? (float)log2((double)d) : 0.0f;
  auto launch = [&](auto half, auto zero, auto factor) {
    constexpr bool DEV = std::is_pointer_v<decltype(factor)>;
    if (ema)
      adam_sparse_ema_kernel<half(), zero(), DEV><<<grid, kThreads, 0, hs>>>(n, master, p16, grads, m, v, param_steps, ema_acc, ema_stamps, ema->state,
                                                                             opt->lr_factor, lr, wd, skip, beta1, beta2, eps, factor, l2b1, l2b2, d,
                                                                             omd, l2d);
    else
      adam_sparse_opt_kernel<half(), zero(), DEV><<<grid, kThreads, 0, hs>>>(n, master, p16, grads, m, v, param_steps, opt->lr_factor, lr, wd, skip,
                                                                             beta1, beta2, eps, factor, l2b1, l2b2);
  };
  with_grad_flags(grad_flags, [&](auto half, auto zero) {
    if (scaler) launch(half, zero, static_cast<const float*>(&scaler->state->multiplier)); else launch(half, zero, 1.0f / loss_scale);
  });
  RTXN_LAUNCH_CHECK(ema ? "adam_sparse_ema_kernel" : scaler ? "adam_sparse_opt_kernel (device multiplier)" : "adam_sparse_opt_kernel");
  return RTXN_OK;
}


int check_schedule(const rtxn_lr_schedule& s, const char* who) {
  RTXN_REQUIRE(s.kind == RTXN_LR_CONSTANT || s.kind == RTXN_LR_EXPONENTIAL || s.kind == RTXN_LR_COSINE,
               "%s: schedule.kind = %d (RTXN_LR_CONSTANT, _EXPONENTIAL or _COSINE)", who, s.kind);
  RTXN_REQUIRE(s.ratio > 0.0f && s.ratio <= 1.0f, "%s: schedule.ratio = %g outside (0, 1]", who, (double)s.ratio);
  RTXN_REQUIRE(s.kind == RTXN_LR_CONSTANT || s.decay_steps >= 1, "%s: schedule.decay_steps = %d (>= 1 unless the kind is RTXN_LR_CONSTANT)", who,
               s.decay_steps);
  RTXN_REQUIRE(s.warmup_steps >= 0, "%s: schedule.warmup_steps = %d < 0", who, s.warmup_steps);
  RTXN_REQUIRE(s.decay_start >= 0, "%s: schedule.decay_start = %d < 0", who, s.decay_start);
  RTXN_REQUIRE(!s.staircase || s.kind == RTXN_LR_EXPONENTIAL, "%s: schedule.staircase is set with kind %d: RTXN_LR_EXPONENTIAL only", who, s.kind);
  return RTXN_OK;
}

}  // namespace

int rtxn::check_optimizer_options(const rtxn_optimizer_options* opt, const char* who, bool need_buffers, bool* active) {
  *active = false;
  if (!opt) return RTXN_OK;
  const int rc = check_schedule(opt->schedule, who);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(std::isfinite(opt->weight_decay) && opt->weight_decay >= 0.0f, "%s: opt->weight_decay = %g (finite, >= 0)", who,
               (double)opt->weight_decay);
  const bool scheduled = opt->schedule.kind != RTXN_LR_CONSTANT || opt->schedule.warmup_steps > 0;
  if (!(scheduled || opt->weight_decay > 0.0f || opt->skip_nonfinite)) return RTXN_OK;
  if (need_buffers) {
    RTXN_REQUIRE(opt->lr_factor, "%s: opt->lr_factor is NULL: the schedule's factor is handed from the rate kernel to the optimizer through it", who);
    RTXN_REQUIRE(!opt->skip_nonfinite || opt->guard, "%s: opt->guard is NULL with opt->skip_nonfinite set", who);
  }
  *active = true;
  return RTXN_OK;
}

extern "C" float rtxn_lr_schedule_factor(const rtxn_lr_schedule* schedule, int step) {
  if (!schedule || step < 1) {
    rtxn::set_error("rtxn_lr_schedule_factor: schedule = %p, step = %d", (const void*)schedule, step);
    return -1.0f;
  }
  if (check_schedule(*schedule, "rtxn_lr_schedule_factor") != RTXN_OK) return -1.0f;
  return schedule_factor(*schedule, step);
}

extern "C" int rtxn_optimizer_options_check(const rtxn_optimizer_options* opt) {
  bool active = false;
  return rtxn::check_optimizer_options(opt, "rtxn_optimizer_options_check", false, &active);
}

// what every entry point that takes the EMA asks of it; with_opt: and of the options beside it (lr_factor whether or not anything
// is switched on: under the EMA the rate always comes from the rate kernel)
static int check_ema(const rtxn_weight_ema* ema, const rtxn_optimizer_options* opt, bool with_opt, const char* who) {
  RTXN_REQUIRE(ema, "%s: NULL ema", who);
  RTXN_REQUIRE(std::isfinite(ema->decay) && ema->decay > 0.0f && ema->decay < 1.0f, "%s: ema->decay = %g (finite, strictly inside (0, 1))", who,
               (double)ema->decay);
  if (!with_opt) return RTXN_OK;
  RTXN_REQUIRE(ema->state && ((uintptr_t)ema->state & 3) == 0, "%s: ema->state = %p (NULL or misaligned)", who, (void*)ema->state);
  RTXN_REQUIRE(opt && opt->lr_factor, "%s: the weight EMA needs options that carry lr_factor (opt = %p): its steps take the rate from the rate kernel",
               who, (const void*)opt);
  return RTXN_OK;
}

static int optimizer_rate_impl(const char* who, const rtxn_optimizer_options* opt, const rtxn_weight_ema* ema, int* step, int advance, float lr,
                               float table_lr, float beta1, float beta2, float* effective_lr, float* table_effective_lr, rtxn_stream_t stream) {
  RTXN_REQUIRE(opt, "%s: NULL options", who);
  bool active = false;
  const int rc = rtxn::check_optimizer_options(opt, who, false, &active);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(opt->lr_factor && (!opt->skip_nonfinite || opt->guard), "%s: opt->lr_factor = %p, opt->guard = %p", who, (void*)opt->lr_factor,
               (void*)opt->guard);
  RTXN_REQUIRE(step && effective_lr, "%s: step = %p, effective_lr = %p", who, (void*)step, (void*)effective_lr);
  ADAM_TRY(check_betas(who, beta1, beta2));
  RTXN_DEVICE_OR_FAIL();
  optimizer_rate_kernel<<<1, 1, 0, rtxn::as_stream(stream)>>>(step, advance, opt->schedule, lr, table_lr, beta1, beta2, effective_lr,
                                                              table_effective_lr, opt->lr_factor, opt->skip_nonfinite ? opt->guard : nullptr,
                                                              ema ? ema->state : nullptr, ema ? ema->decay : 0.0f);
  RTXN_LAUNCH_CHECK("optimizer_rate_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_optimizer_rate(const rtxn_optimizer_options* opt, int* step, int advance, float lr, float table_lr, float beta1, float beta2,
                                   float* effective_lr, float* table_effective_lr, rtxn_stream_t stream) {
  return optimizer_rate_impl("rtxn_optimizer_rate", opt, nullptr, step, advance, lr, table_lr, beta1, beta2, effective_lr, table_effective_lr, stream);
}

extern "C" int rtxn_optimizer_rate_ema(const rtxn_optimizer_options* opt, const rtxn_weight_ema* ema, int* step, int advance, float lr,
                                       float table_lr, float beta1, float beta2, float* effective_lr, float* table_effective_lr,
                                       rtxn_stream_t stream) {
  const char* who = "rtxn_optimizer_rate_ema";
  if (ema) {
    const int rc = check_ema(ema, opt, true, who);
    if (rc != RTXN_OK) return rc;
  }
  return optimizer_rate_impl(who, opt, ema, step, advance, lr, table_lr, beta1, beta2, effective_lr, table_effective_lr, stream);
}

extern "C" int rtxn_check_gradients(const rtxn_grad_buffer* buffers, int n_buffers, unsigned* flag, rtxn_stream_t stream) {
  const char* who = "rtxn_check_gradients";
  RTXN_REQUIRE(n_buffers >= 0 && n_buffers <= RTXN_MAX_GRAD_BUFFERS && (buffers || n_buffers == 0), "%s: n_buffers = %d (0 .. %d), buffers = %p", who,
               n_buffers, (int)RTXN_MAX_GRAD_BUFFERS, (const void*)buffers);
  RTXN_REQUIRE(flag, "%s: NULL flag", who);
  GradList L = {};
  int k = 0;
  long most = 0;                                                // 16-byte words of the largest buffer
  for (int i = 0; i < n_buffers; ++i) {
    const rtxn_grad_buffer& b = buffers[i];
    RTXN_REQUIRE(b.count >= 0, "%s: buffers[%d].count = %ld", who, i, b.count);
    if (b.count == 0) continue;
    const int esize = b.is_fp16 ? 2 : 4;
    RTXN_REQUIRE(b.data && ((uintptr_t)b.data & (uintptr_t)(esize - 1)) == 0, "%s: buffers[%d].data = %p (NULL, or not aligned to its element)", who,
                 i, b.data);
    L.data[k] = b.data;
    L.count[k] = b.count;
    L.is_fp16[k] = b.is_fp16 != 0;
    const long words = (b.count * esize + 15) / 16;
    most = words > most ? words : most;
    ++k;
  }
  RTXN_DEVICE_OR_FAIL();
  if (k == 0) return RTXN_OK;
  const long blocks = (most + 4 * kThreads - 1) / (4 * kThreads);          // four 16-byte words per lane and trip
  const dim3 grid((unsigned)(blocks > 2048 ? 2048 : blocks), (unsigned)k);
  check_gradients_kernel<<<grid, kThreads, 0, rtxn::as_stream(stream)>>>(L, flag);
  RTXN_LAUNCH_CHECK("check_gradients_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_adam_step(long n, float* master, void* params_fp16, const float* grads, float* m, float* v, int step,
                              float lr, float beta1, float beta2, float eps, float loss_scale, rtxn_stream_t stream) {
  RTXN_REQUIRE(n >= 0 && step >= 1, "rtxn_adam_step: n = %ld, step = %d", n, step);
  return adam_impl("rtxn_adam_step", n, master, params_fp16, const_cast<float*>(grads), 0, m, v, adam_lr_eff(lr, beta1, beta2, step), nullptr, beta1,
                   beta2, eps, loss_scale, stream);
}

extern "C" int rtxn_adam_step_half_grads(long n, float* master, void* params_fp16, const void* grads_fp16, float* m, float* v,
                                         int step, float lr, float beta1, float beta2, float eps, float loss_scale,
                                         rtxn_stream_t stream) {
  RTXN_REQUIRE(n >= 0 && step >= 1, "rtxn_adam_step_half_grads: n = %ld, step = %d", n, step);
  return adam_impl("rtxn_adam_step_half_grads", n, master, params_fp16, const_cast<void*>(grads_fp16), RTXN_ADAM_GRADS_FP16, m, v,
                   adam_lr_eff(lr, beta1, beta2, step), nullptr, beta1, beta2, eps, loss_scale, stream);
}

extern "C" float rtxn_adam_effective_lr(float lr, float beta1, float beta2, int step) {
  return step >= 1 ? adam_lr_eff(lr, beta1, beta2, step) : 0.0f;
}

extern "C" int rtxn_adam_step_captured(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m,
                                       float* v, const float* effective_lr, float beta1, float beta2, float eps, float loss_scale,
                                       rtxn_stream_t stream) {
  const char* who = "rtxn_adam_step_captured";
  RTXN_REQUIRE(n >= 0 && effective_lr, "%s: n = %ld, effective_lr = %p", who, n, (const void*)effective_lr);
  ADAM_TRY(check_grad_flags(who, grad_flags, false));
  return adam_impl(who, n, master, params_fp16, grads, grad_flags, m, v, 0.0f, effective_lr, beta1, beta2, eps, loss_scale, stream);
}

extern "C" int rtxn_adam_step_sparse(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                                     unsigned* param_steps, float lr, float beta1, float beta2, float eps, float loss_scale,
                                     rtxn_stream_t stream) {
  const char* who = "rtxn_adam_step_sparse";
  RTXN_REQUIRE(n >= 0, "%s: n = %ld", who, n);
  ADAM_TRY(check_grad_flags(who, grad_flags, false));
  RTXN_REQUIRE(loss_scale != 0.0f, "%s: loss_scale = 0", who);
  RTXN_DEVICE_OR_FAIL();
  if (n == 0) return RTXN_OK;
  RTXN_REQUIRE(master && params_fp16 && grads && m && v && param_steps, "%s: NULL buffer", who);
  ADAM_TRY(check_betas(who, beta1, beta2));
  const float l2b1 = (float)log2((double)beta1), l2b2 = (float)log2((double)beta2);
  with_grad_flags(grad_flags, [&](auto half, auto zero) {
    adam_sparse_kernel<half(), zero()><<<adam_sparse_grid(n), kThreads, 0, rtxn::as_stream(stream)>>>(
        n, master, static_cast<__half*>(params_fp16), grads, m, v, param_steps, lr, beta1, beta2, eps, 1.0f / loss_scale, l2b1, l2b2);
  });
  RTXN_LAUNCH_CHECK("adam_sparse_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_adam_step_opt(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                                  const float* effective_lr, float lr, float beta1, float beta2, float eps, float loss_scale,
                                  const rtxn_optimizer_options* opt, rtxn_stream_t stream) {
  const char* who = "rtxn_adam_step_opt";
  bool active = false;
  ADAM_TRY(rtxn::check_optimizer_options(opt, who, true, &active));
  ADAM_TRY(check_grad_flags(who, grad_flags, true));
  if (!active) return rtxn_adam_step_captured(n, master, params_fp16, grads, grad_flags & 3, m, v, effective_lr, beta1, beta2, eps, loss_scale, stream);
  return adam_dense_options(who, n, master, params_fp16, grads, grad_flags, m, v, effective_lr, lr, beta1, beta2, eps, loss_scale, opt, nullptr, nullptr,
                            nullptr, stream);
}

extern "C" int rtxn_adam_step_sparse_opt(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                                         unsigned* param_steps, float lr, float beta1, float beta2, float eps, float loss_scale,
                                         const rtxn_optimizer_options* opt, rtxn_stream_t stream) {
  const char* who = "rtxn_adam_step_sparse_opt";
  bool active = false;
  ADAM_TRY(rtxn::check_optimizer_options(opt, who, true, &active));
  ADAM_TRY(check_grad_flags(who, grad_flags, true));
  if (!active) return rtxn_adam_step_sparse(n, master, params_fp16, grads, grad_flags & 3, m, v, param_steps, lr, beta1, beta2, eps, loss_scale, stream);
  return adam_sparse_options(who, n, master, params_fp16, grads, grad_flags, m, v, param_steps, lr, beta1, beta2, eps, loss_scale, opt, nullptr, nullptr,
                             nullptr, nullptr, stream);
}

// ------------------------------------------------------------------------- dynamic loss scale, gradient-norm clipping
namespace {

// The scaler's state machine of include/rtxn.h, the one restatement host and device share (as schedule_factor is): st holds
// the scale the step's gradients were made with; bad: the non-finite flag; sumsq: the sum of squares of the scaled gradients.
__host__ __device__ inline void loss_scaler_advance(const rtxn_loss_scaler& c, rtxn_loss_scaler_state& st, bool bad, double sumsq, float D) {
  const float s = st.scale;
  if (bad) {
    st.scale = fmaxf(c.min_scale, s * c.backoff);
    st.good = 0;
    st.backoffs += 1u;
    return;
  }
  const float norm = (float)(sqrt(sumsq) / ((double)s * (double)D));
  const float coef = c.max_grad_norm > 0.0f ? fminf(1.0f, c.max_grad_norm / (norm + 1e-6f)) : 1.0f;
  st.multiplier = coef * (1.0f / (s * D));
  st.grad_norm = norm;
  st.clipped += coef < 1.0f ? 1u : 0u;
  st.good += 1;
  if (st.good >= c.growth_interval) {
    const float grown = fminf(c.max_scale, s * c.growth);
    st.good = 0;
    st.growths += grown != s ? 1u : 0u;
    st.scale = grown;
  }
}

// the buffers of a statistics launch: GradList and each buffer's own block count, a function of its count and type alone
struct StatList {
  GradList g;
  int blocks[RTXN_MAX_GRAD_BUFFERS];
};

__device__ __forceinline__ double square_d(float x) {
  const double d = (double)x;
  return d * d;
}
struct StatF32 {
  __device__ __forceinline__ void operator()(unsigned w, bool& bad, double& s) const {
    bad |= nonfinite_f32(w);
    s += square_d(__uint_as_float(w));
  }
};
struct StatH2 {
  __device__ __forceinline__ void operator()(unsigned w, bool& bad, double& s) const {
    bad |= nonfinite_h2(w);
    s += square_d((float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)));
    s += square_d((float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)));
  }
};

// any_word with the sums: the four loads of a trip feed four sums of their own, joined pairwise at the end -- a fixed order
template <typename Word>
__device__ __forceinline__ double stat_words(const uint4* __restrict__ q, long body, long gid, long stride, Word word, bool& bad) {
  double sa = 0.0, sb = 0.0, sc = 0.0, sd = 0.0;
  long k = gid;
  for (; k + 3 * stride < body; k += 4 * stride) {
    const uint4 a = q[k], b = q[k + stride], c = q[k + 2 * stride], d = q[k + 3 * stride];
    word(a.x, bad, sa); word(a.y, bad, sa); word(a.z, bad, sa); word(a.w, bad, sa);
    word(b.x, bad, sb); word(b.y, bad, sb); word(b.z, bad, sb); word(b.w, bad, sb);
    word(c.x, bad, sc); word(c.y, bad, sc); word(c.z, bad, sc); word(c.w, bad, sc);
    word(d.x, bad, sd); word(d.y, bad, sd); word(d.z, bad, sd); word(d.w, bad, sd);
  }
  for (; k < body; k += stride) {
    const uint4 w = q[k];
    word(w.x, bad, sa); word(w.y, bad, sa); word(w.z, bad, sa); word(w.w, bad, sa);
  }
  return (sa + sb) + (sc + sd);
}

// check_gradients_kernel's pass and traffic shape; besides the OR every lane sums the squares of what it reads in double, in
// visiting order.  blockIdx.y: the buffer, over L.blocks[b] blocks of its own (a block past them leaves whole).  The sums meet
// in a fixed order -- wave (the DPP scan), then the block's four waves through LDS -- and one double per block is stored at
// partials[buffer][block]: no atomic touches them.  The flag stays one atomic OR per wave after a ballot.
__global__ __launch_bounds__(kThreads) void gradient_statistics_kernel(StatList L, unsigned* __restrict__ flag, double* __restrict__ partials) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.y;
  const int nb = L.blocks[b];
  if ((int)blockIdx.x >= nb) return;
  const long n = L.g.count[b];
  const long gid = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)nb * kThreads;
  const uintptr_t base = (uintptr_t)L.g.data[b];
  const int esize = L.g.is_fp16[b] ? 2 : 4, per16 = 16 / esize;
  long head = (long)(((16u - (unsigned)(base & 15u)) & 15u) / (unsigned)esize);
  if (head > n) head = n;
  const long body = (n - head) / per16, tail = head + body * per16;
  bool bad = false;
  double sum = 0.0;
  if (L.g.is_fp16[b]) {
    const unsigned short* h = reinterpret_cast<const unsigned short*>(base);
    for (long i = gid; i < head; i += stride) {
      bad |= (h[i] & 0x7c00u) == 0x7c00u;
      sum += square_d((float)__builtin_bit_cast(_Float16, h[i]));
    }
    sum += stat_words(reinterpret_cast<const uint4*>(h + head), body, gid, stride, StatH2(), bad);
    for (long i = tail + gid; i < n; i += stride) {
      bad |= (h[i] & 0x7c00u) == 0x7c00u;
      sum += square_d((float)__builtin_bit_cast(_Float16, h[i]));
    }
  } else {
    const unsigned* f = reinterpret_cast<const unsigned*>(base);
    for (long i = gid; i < head; i += stride) StatF32()(f[i], bad, sum);
    sum += stat_words(reinterpret_cast<const uint4*>(f + head), body, gid, stride, StatF32(), bad);
    for (long i = tail + gid; i < n; i += stride) StatF32()(f[i], bad, sum);
  }
  const bool any = __ballot(bad) != 0;
  if (any && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
  const double wsum = wave_sum_d(sum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) partials[(long)b * RTXN_GRAD_STATS_MAX_BLOCKS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// optimizer_rate_kernel's sibling, one block.  Thread t sums the partials t, t + 256, ... of each buffer in turn, the 256 sums
// meet in a halving tree through LDS; thread 0 then does the rate kernel's work and moves the scaler's state.  One launch,
// shared by every stepping path: their scales, multipliers and rates are the same bits by construction.
__global__ __launch_bounds__(kThreads) void loss_scaler_kernel(int* step, int advance, rtxn_lr_schedule s, float lr, float table_lr, float beta1,
                                                               float beta2, float* lr_eff, float* table_lr_eff, float* factor_out,
                                                               unsigned* guard, rtxn_loss_scaler cfg, float divisor, StatList L,
                                                               rtxn_ema_state* ema, float ema_decay) {
  __shared__ double red[kThreads];
  double acc = 0.0;
  for (int b = 0; b < RTXN_MAX_GRAD_BUFFERS; ++b)
    for (int j = threadIdx.x; j < L.blocks[b]; j += kThreads) acc += cfg.partials[(long)b * RTXN_GRAD_STATS_MAX_BLOCKS + j];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned bad = rate_update(step, advance, s, lr, table_lr, beta1, beta2, lr_eff, table_lr_eff, factor_out, guard);
    rtxn_loss_scaler_state st = *cfg.state;
    loss_scaler_advance(cfg, st, bad != 0u, red[0], divisor);
    *cfg.state = st;
    ema_advance(ema, ema_decay, bad, advance);
  }
}

bool power_of_two(float x) {
  int e;
  return std::isfinite(x) && x > 0.0f && frexpf(x, &e) == 0.5f;
}

// rtxn_check_gradients' argument checks and compaction (buffers with count 0 are skipped), plus each buffer's block count:
// four 16-byte words per lane and trip, at most RTXN_GRAD_STATS_MAX_BLOCKS.  need_data: the pointers are checked as well.
int make_stat_list(const char* who, const rtxn_grad_buffer* buffers, int n_buffers, bool need_data, StatList* out, int* k_out, int* most_out) {
  RTXN_REQUIRE(n_buffers >= 0 && n_buffers <= RTXN_MAX_GRAD_BUFFERS && (buffers || n_buffers == 0), "%s: n_buffers = %d (0 .. %d), buffers = %p", who,
               n_buffers, (int)RTXN_MAX_GRAD_BUFFERS, (const void*)buffers);
  StatList L = {};
  int k = 0, most = 0;
  for (int i = 0; i < n_buffers; ++i) {
    const rtxn_grad_buffer& b = buffers[i];
    RTXN_REQUIRE(b.count >= 0, "%s: buffers[%d].count = %ld", who, i, b.count);
    if (b.count == 0) continue;
    const int esize = b.is_fp16 ? 2 : 4;
    if (need_data)
      RTXN_REQUIRE(b.data && ((uintptr_t)b.data & (uintptr_t)(esize - 1)) == 0, "%s: buffers[%d].data = %p (NULL, or not aligned to its element)",
                   who, i, b.data);
    L.g.data[k] = b.data;
    L.g.count[k] = b.count;
    L.g.is_fp16[k] = b.is_fp16 != 0;
    const long words = (b.count * esize + 15) / 16;
    const long blocks = (words + 4 * kThreads - 1) / (4 * kThreads);
    L.blocks[k] = (int)(blocks > RTXN_GRAD_STATS_MAX_BLOCKS ? RTXN_GRAD_STATS_MAX_BLOCKS : blocks);
    most = L.blocks[k] > most ? L.blocks[k] : most;
    ++k;
  }
  *out = L;
  *k_out = k;
  *most_out = most;
  return RTXN_OK;
}

// what every entry point that takes the scaler asks of it and of the options beside it
int check_scaled(const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const char* who) {
  RTXN_REQUIRE(scaler, "%s: NULL scaler", who);
  int rc = rtxn::check_loss_scaler(scaler, who, true);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(opt, "%s: NULL options: the loss scaler needs the non-finite guard (opt->skip_nonfinite, opt->guard)", who);
  bool active = false;
  rc = rtxn::check_optimizer_options(opt, who, true, &active);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(opt->skip_nonfinite && opt->guard && opt->lr_factor,
               "%s: the loss scaler needs opt->skip_nonfinite with opt->guard and opt->lr_factor (skip_nonfinite = %d, guard = %p, lr_factor = %p)", who,
               opt->skip_nonfinite, (void*)opt->guard, (void*)opt->lr_factor);
  return RTXN_OK;
}

}  // namespace

int rtxn::check_loss_scaler(const rtxn_loss_scaler* c, const char* who, bool need_buffers) {
  RTXN_REQUIRE(c, "%s: NULL scaler", who);
  RTXN_REQUIRE(power_of_two(c->init_scale), "%s: scaler->init_scale = %g is not a power of two", who, (double)c->init_scale);
  RTXN_REQUIRE(power_of_two(c->growth) && c->growth >= 1.0f, "%s: scaler->growth = %g (a power of two >= 1)", who, (double)c->growth);
  RTXN_REQUIRE(power_of_two(c->backoff) && c->backoff < 1.0f, "%s: scaler->backoff = %g (a power of two in (0, 1))", who, (double)c->backoff);
  RTXN_REQUIRE(power_of_two(c->min_scale), "%s: scaler->min_scale = %g is not a power of two", who, (double)c->min_scale);
  RTXN_REQUIRE(power_of_two(c->max_scale), "%s: scaler->max_scale = %g is not a power of two", who, (double)c->max_scale);
  RTXN_REQUIRE(c->min_scale <= c->init_scale && c->init_scale <= c->max_scale, "%s: scaler->min_scale = %g <= init_scale = %g <= max_scale = %g does not hold",
               who, (double)c->min_scale, (double)c->init_scale, (double)c->max_scale);
  RTXN_REQUIRE(c->growth_interval >= 1, "%s: scaler->growth_interval = %d < 1", who, c->growth_interval);
  RTXN_REQUIRE(std::isfinite(c->max_grad_norm) && c->max_grad_norm >= 0.0f, "%s: scaler->max_grad_norm = %g (finite, >= 0; 0: no clipping)", who,
               (double)c->max_grad_norm);
  if (need_buffers)
    RTXN_REQUIRE(c->state && c->partials && ((uintptr_t)c->partials & 7) == 0 && ((uintptr_t)c->state & 3) == 0,
                 "%s: scaler->state = %p, scaler->partials = %p (NULL or misaligned)", who, (void*)c->state, (void*)c->partials);
  return RTXN_OK;
}

extern "C" int rtxn_loss_scaler_check(const rtxn_loss_scaler* scaler) { return rtxn::check_loss_scaler(scaler, "rtxn_loss_scaler_check", false); }

extern "C" size_t rtxn_loss_scaler_workspace_bytes(void) { return sizeof(double) * RTXN_MAX_GRAD_BUFFERS * RTXN_GRAD_STATS_MAX_BLOCKS; }

extern "C" int rtxn_loss_scaler_init_state(const rtxn_loss_scaler* scaler, rtxn_loss_scaler_state* state_out) {
  const int rc = rtxn::check_loss_scaler(scaler, "rtxn_loss_scaler_init_state", false);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(state_out, "rtxn_loss_scaler_init_state: NULL state_out");
  rtxn_loss_scaler_state st = {};
  st.scale = scaler->init_scale;
  st.multiplier = 1.0f / scaler->init_scale;
  *state_out = st;
  return RTXN_OK;
}

extern "C" int rtxn_loss_scaler_advance(const rtxn_loss_scaler* scaler, const rtxn_loss_scaler_state* state_in, int flag, double sumsq,
                                        float divisor, rtxn_loss_scaler_state* state_out) {
  const char* who = "rtxn_loss_scaler_advance";
  const int rc = rtxn::check_loss_scaler(scaler, who, false);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(state_in && state_out, "%s: state_in = %p, state_out = %p", who, (const void*)state_in, (void*)state_out);
  RTXN_REQUIRE(state_in->scale > 0.0f && divisor > 0.0f && sumsq >= 0.0, "%s: scale = %g, divisor = %g, sumsq = %g", who, (double)state_in->scale,
               (double)divisor, sumsq);
  rtxn_loss_scaler_state st = *state_in;
  loss_scaler_advance(*scaler, st, flag != 0, sumsq, divisor);
  *state_out = st;
  return RTXN_OK;
}

extern "C" int rtxn_gradient_statistics(const rtxn_grad_buffer* buffers, int n_buffers, unsigned* flag, const rtxn_loss_scaler* scaler,
                                        rtxn_stream_t stream) {
  const char* who = "rtxn_gradient_statistics";
  int rc = rtxn::check_loss_scaler(scaler, who, true);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(flag, "%s: NULL flag", who);
  StatList L;
  int k = 0, most = 0;
  rc = make_stat_list(who, buffers, n_buffers, true, &L, &k, &most);
  if (rc != RTXN_OK) return rc;
  RTXN_DEVICE_OR_FAIL();
  if (k == 0) return RTXN_OK;
  gradient_statistics_kernel<<<dim3((unsigned)most, (unsigned)k), kThreads, 0, rtxn::as_stream(stream)>>>(L, flag, scaler->partials);
  RTXN_LAUNCH_CHECK("gradient_statistics_kernel");
  return RTXN_OK;
}

static int loss_scaler_step_impl(const char* who, const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema,
                                 const rtxn_grad_buffer* buffers, int n_buffers, int* step, int advance, float lr, float table_lr, float beta1,
                                 float beta2, float* effective_lr, float* table_effective_lr, float divisor, rtxn_stream_t stream) {
  int rc = check_scaled(opt, scaler, who);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(step && effective_lr, "%s: step = %p, effective_lr = %p", who, (void*)step, (void*)effective_lr);
  ADAM_TRY(check_betas(who, beta1, beta2));
  RTXN_REQUIRE(divisor > 0.0f && std::isfinite(divisor), "%s: divisor = %g", who, (double)divisor);
  StatList L;
  int k = 0, most = 0;
  rc = make_stat_list(who, buffers, n_buffers, false, &L, &k, &most);
  if (rc != RTXN_OK) return rc;
  RTXN_DEVICE_OR_FAIL();
  loss_scaler_kernel<<<1, kThreads, 0, rtxn::as_stream(stream)>>>(step, advance, opt->schedule, lr, table_lr, beta1, beta2, effective_lr,
                                                                  table_effective_lr, opt->lr_factor, opt->guard, *scaler, divisor, L,
                                                                  ema ? ema->state : nullptr, ema ? ema->decay : 0.0f);
  RTXN_LAUNCH_CHECK("loss_scaler_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_loss_scaler_step(const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_grad_buffer* buffers,
                                     int n_buffers, int* step, int advance, float lr, float table_lr, float beta1, float beta2,
                                     float* effective_lr, float* table_effective_lr, float divisor, rtxn_stream_t stream) {
  return loss_scaler_step_impl("rtxn_loss_scaler_step", opt, scaler, nullptr, buffers, n_buffers, step, advance, lr, table_lr, beta1, beta2,
                               effective_lr, table_effective_lr, divisor, stream);
}

extern "C" int rtxn_loss_scaler_step_ema(const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema,
                                         const rtxn_grad_buffer* buffers, int n_buffers, int* step, int advance, float lr, float table_lr,
                                         float beta1, float beta2, float* effective_lr, float* table_effective_lr, float divisor,
                                         rtxn_stream_t stream) {
  const char* who = "rtxn_loss_scaler_step_ema";
  if (ema) {
    const int rc = check_ema(ema, opt, true, who);
    if (rc != RTXN_OK) return rc;
  }
  return loss_scaler_step_impl(who, opt, scaler, ema, buffers, n_buffers, step, advance, lr, table_lr, beta1, beta2, effective_lr,
                               table_effective_lr, divisor, stream);
}

extern "C" int rtxn_adam_step_scaled(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                                     const float* effective_lr, float lr, float beta1, float beta2, float eps,
                                     const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, rtxn_stream_t stream) {
  const char* who = "rtxn_adam_step_scaled";
  ADAM_TRY(check_scaled(opt, scaler, who));
  ADAM_TRY(check_grad_flags(who, grad_flags, true));
  return adam_dense_options(who, n, master, params_fp16, grads, grad_flags, m, v, effective_lr, lr, beta1, beta2, eps, 0.0f, opt, scaler, nullptr, nullptr,
                            stream);
}

extern "C" int rtxn_adam_step_sparse_scaled(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                                            unsigned* param_steps, float lr, float beta1, float beta2, float eps,
                                            const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, rtxn_stream_t stream) {
  const char* who = "rtxn_adam_step_sparse_scaled";
  ADAM_TRY(check_scaled(opt, scaler, who));
  ADAM_TRY(check_grad_flags(who, grad_flags, true));
  return adam_sparse_options(who, n, master, params_fp16, grads, grad_flags, m, v, param_steps, lr, beta1, beta2, eps, 0.0f, opt, scaler, nullptr, nullptr,
                             nullptr, stream);
}

// ------------------------------------------------------------------------- exponential moving average of the weights
namespace {

// The read-out: catch_up(s, w, u - e) correction(u), or w itself at u = 0.  Pure -- it stores only the outputs.  One 16-byte
// word per lane and array, and two quads per trip: four to six independent loads in flight per lane (one load in flight per lane
// left a pass of this shape at half the HBM rate).  LAZY: with stamps.
template <bool LAZY>
__global__ __launch_bounds__(kThreads) void ema_weights_kernel(long n, const float* __restrict__ master, const float* __restrict__ acc,
                                                               const unsigned* __restrict__ stamps, const rtxn_ema_state* __restrict__ ema,
                                                               float log2_d, float* __restrict__ out32, __half* __restrict__ out16) {
  const unsigned u = ema->updates;
  const float corr = ema->correction;
  auto one = [&](float w, float s, unsigned e) { return u == 0u ? w : (LAZY ? ema_catch_up(s, w, u - e, log2_d) : s) * corr; };
  const bool vec = (((uintptr_t)master | (uintptr_t)acc | (uintptr_t)stamps | (uintptr_t)out32) & 15) == 0 && ((uintptr_t)out16 & 7) == 0;
  const long n4 = vec ? n / 4 : 0;
  const long first = (long)blockIdx.x * kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
  auto quad = [&](float4 w, float4 s, uint4 e, long q) {
    const float4 o = make_float4(one(w.x, s.x, e.x), one(w.y, s.y, e.y), one(w.z, s.z, e.z), one(w.w, s.w, e.w));
    if (out32) reinterpret_cast<float4*>(out32)[q] = o;
    if (out16) {
      const half4v h = {(_Float16)o.x, (_Float16)o.y, (_Float16)o.z, (_Float16)o.w};
      reinterpret_cast<half4v*>(out16)[q] = h;
    }
  };
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  long q = first;
  for (; q + stride < n4; q += 2 * stride) {
    const float4 wa = reinterpret_cast<const float4*>(master)[q], wb = reinterpret_cast<const float4*>(master)[q + stride];
    const float4 sa = reinterpret_cast<const float4*>(acc)[q], sb = reinterpret_cast<const float4*>(acc)[q + stride];
    const uint4 ea = LAZY ? reinterpret_cast<const uint4*>(stamps)[q] : zero, eb = LAZY ? reinterpret_cast<const uint4*>(stamps)[q + stride] : zero;
    quad(wa, sa, ea, q);
    quad(wb, sb, eb, q + stride);
  }
  for (; q < n4; q += stride)
    quad(reinterpret_cast<const float4*>(master)[q], reinterpret_cast<const float4*>(acc)[q], LAZY ? reinterpret_cast<const uint4*>(stamps)[q] : zero, q);
  for (long i = 4 * n4 + first; i < n; i += stride) {
    const float o = one(master[i], acc[i], LAZY ? stamps[i] : 0u);
    if (out32) out32[i] = o;
    if (out16) out16[i] = __float2half(o);
  }
}

// what an _ema Adam call asks in front of its launch path: the EMA, the scaler with the options it needs or the options alone and
// the loss scale by value, then the flags
int check_ema_step(const char* who, const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, float loss_scale,
                   int grad_flags) {
  ADAM_TRY(check_ema(ema, opt, true, who));
  if (scaler) {
    ADAM_TRY(check_scaled(opt, scaler, who));
  } else {
    bool active = false;
    ADAM_TRY(rtxn::check_optimizer_options(opt, who, true, &active));      // with skip_nonfinite set this asks for the guard too
    RTXN_REQUIRE(loss_scale != 0.0f, "%s: loss_scale = 0", who);
  }
  return check_grad_flags(who, grad_flags, true);
}

}  // namespace

extern "C" int rtxn_weight_ema_check(const rtxn_weight_ema* ema) { return ema ? check_ema(ema, nullptr, false, "rtxn_weight_ema_check") : RTXN_OK; }

extern "C" float rtxn_ema_catch_up(float s, float w, unsigned gap, float decay) {
  if (!(std::isfinite(decay) && decay > 0.0f && decay < 1.0f)) {
    rtxn::set_error("rtxn_ema_catch_up: decay = %g (finite, strictly inside (0, 1))", (double)decay);
    return NAN;
  }
  return ema_catch_up(s, w, gap, (float)log2((double)decay));
}

extern "C" float rtxn_ema_correction(float decay, unsigned updates) {
  if (!(std::isfinite(decay) && decay > 0.0f && decay < 1.0f)) {
    rtxn::set_error("rtxn_ema_correction: decay = %g (finite, strictly inside (0, 1))", (double)decay);
    return -1.0f;
  }
  return ema_correction(decay, updates);
}

extern "C" int rtxn_adam_step_ema(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                                  const float* effective_lr, float lr, float beta1, float beta2, float eps, float loss_scale,
                                  const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, float* ema_acc,
                                  rtxn_stream_t stream) {
  const char* who = "rtxn_adam_step_ema";
  if (!ema)
    return scaler ? rtxn_adam_step_scaled(n, master, params_fp16, grads, grad_flags, m, v, effective_lr, lr, beta1, beta2, eps, opt, scaler, stream)
                  : rtxn_adam_step_opt(n, master, params_fp16, grads, grad_flags, m, v, effective_lr, lr, beta1, beta2, eps, loss_scale, opt, stream);
  ADAM_TRY(check_ema_step(who, opt, scaler, ema, loss_scale, grad_flags));
  return adam_dense_options(who, n, master, params_fp16, grads, grad_flags, m, v, effective_lr, lr, beta1, beta2, eps, loss_scale, opt, scaler, ema,
                            ema_acc, stream);
}

extern "C" int rtxn_adam_step_sparse_ema(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                                         unsigned* param_steps, float lr, float beta1, float beta2, float eps, float loss_scale,
                                         const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema,
                                         float* ema_acc, unsigned* ema_stamps, rtxn_stream_t stream) {
  const char* who = "rtxn_adam_step_sparse_ema";
  if (!ema)
    return scaler ? rtxn_adam_step_sparse_scaled(n, master, params_fp16, grads, grad_flags, m, v, param_steps, lr, beta1, beta2, eps, opt, scaler, stream)
                  : rtxn_adam_step_sparse_opt(n, master, params_fp16, grads, grad_flags, m, v, param_steps, lr, beta1, beta2, eps, loss_scale, opt,
                                              stream);
  ADAM_TRY(check_ema_step(who, opt, scaler, ema, loss_scale, grad_flags));
  return adam_sparse_options(who, n, master, params_fp16, grads, grad_flags, m, v, param_steps, lr, beta1, beta2, eps, loss_scale, opt, scaler, ema, ema_acc,
                             ema_stamps, stream);
}

extern "C" int rtxn_ema_weights(long n, const float* master, const float* ema_acc, const unsigned* stamps, const rtxn_ema_state* state, float decay,
                                float* out_f32, void* out_f16, rtxn_stream_t stream) {
  const char* who = "rtxn_ema_weights";
  RTXN_REQUIRE(std::isfinite(decay) && decay > 0.0f && decay < 1.0f, "%s: decay = %g (finite, strictly inside (0, 1))", who, (double)decay);
  RTXN_REQUIRE(state && ((uintptr_t)state & 3) == 0, "%s: state = %p (NULL or misaligned)", who, (const void*)state);
  RTXN_REQUIRE(n >= 0, "%s: n = %ld", who, n);
  RTXN_REQUIRE(out_f32 || out_f16, "%s: neither out_f32 nor out_f16", who);
  RTXN_DEVICE_OR_FAIL();
  if (n == 0) return RTXN_OK;
  RTXN_REQUIRE(master && ema_acc, "%s: master = %p, ema_acc = %p", who, (const void*)master, (const void*)ema_acc);
  const long blocks = ((n + 3) / 4 + 2 * kThreads - 1) / (2 * kThreads);            // two quads per lane and trip
  const unsigned gridx = (unsigned)(blocks > 4096 ? 4096 : blocks);
  const float l2d = (float)log2((double)decay);
  (stamps ? ema_weights_kernel<true> : ema_weights_kernel<false>)<<<gridx, kThreads, 0, rtxn::as_stream(stream)>>>(
      n, master, ema_acc, stamps, state, l2d, out_f32, static_cast<__half*>(out_f16));
  RTXN_LAUNCH_CHECK("ema_weights_kernel");
  return RTXN_OK;
}
