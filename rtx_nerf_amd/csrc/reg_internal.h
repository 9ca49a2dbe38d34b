// The distortion regulariser of rtxn_train_regularizer (include/rtxn.h): what the regularised compositor
// (composite_train.hip) and the fixed-order loss sum behind it (loss.hip) share, so that both form a ray's share of the scalar from the same
// operations, bit for bit (-ffp-contract=off on every side).  Internal to librtxn.so; anonymous namespace, as LossArgs is.
#pragma once
#include "common.h"

namespace {

struct RegArgs {
  float weight;            // lambda_d
  float k;                 // loss_scale lambda_d / n_rays: the factor of q_i in sweep 2 (fp32; no fp16 hand-off)
  const float* t_start;    // per packed segment slot
  const float* t_end;
  float* distortion;       // L_r of every ray (may be NULL); the fixed-order sum reads it when lambda_d > 0
  float* depth;            // sum w m of every ray (may be NULL)
};

// the kernels' argument from the caller's struct; reg: an ACTIVE regulariser, or NULL (all zero: nothing reads it)
inline RegArgs make_reg_args(const rtxn_train_regularizer* reg, float loss_scale, int n_rays) {
  RegArgs ra{};
  if (reg) {
    ra.weight = reg->distortion_weight;
    ra.k = loss_scale * reg->distortion_weight / (float)n_rays;
    ra.t_start = reg->t_start;
    ra.t_end = reg->t_end;
    ra.distortion = reg->distortion;
    ra.depth = reg->depth;
  }
  return ra;
}

// the factor of q_i in a kernel: RegArgs::k as make_reg_args formed it on the host or (DEV: the loss scale is a device word,
// rtxn_loss_scaler) its expression in its order, an IEEE division, from the scale the wave read
template <bool DEV>
__device__ __forceinline__ float reg_k(const RegArgs& ra, float loss_scale, int n_rays) {
  if constexpr (DEV) return loss_scale * ra.weight / (float)n_rays;
  else return ra.k;
}

// midpoint of sub-interval k of a segment (volrender_aux_kernel's depth expression with u0 = 0.5)
__device__ __forceinline__ float reg_midpoint(int k, float rK, float ts, float te) { return fmaf(((float)k + 0.5f) * rK, te - ts, ts); }

// ... and its width: a distance along the ray, free of the t_scale the compositor's step lengths carry
__device__ __forceinline__ float reg_width(float rK, float ts, float te) { return (te - ts) * rK; }

// L_r from the two sums sweep 1 leaves: pair = sum_i w_i (m_i W_<i - M_<i), self = sum_i w_i^2 delta_i
__device__ __forceinline__ float reg_ray_value(float pair, float self) { return 2.0f * pair + self * (1.0f / 3.0f); }

// a ray's share of the loss scalar: (lambda_d / n_rays) L_r
__device__ __forceinline__ float reg_loss_share(float weight, float L, float inv_rays) { return weight * L * inv_rays; }

}  // namespace
