// The depth term of rtxn_train_depth (include/rtxn.h): what the compositor's DEPTH instantiations
// (composite_train.hip) and the fixed-order loss sum behind them (loss.hip) share, so that both form a ray's share of the scalar
// from the same operations, bit for bit (-ffp-contract=off on every side).  Internal to librtxn.so; anonymous namespace, as
// RegArgs is.
#pragma once
#include <type_traits>

#include "common.h"
#include "loss_internal.h"
#include "reg_internal.h"

namespace {

struct DepthArgs {
  float weight;            // lambda_z
  int kind;                // rtxn_loss_kind: L2 | L1 | HUBER
  float param;             // HUBER: delta
  float k;                 // loss_scale lambda_z / n_rays: the factor of l'(e_r) in g_D (fp32; no fp16 hand-off)
  const float* target;     // z_r of every ray
  float* depth;            // D_r of every ray (may be NULL); the fixed-order sum reads it when lambda_z > 0
  float* depth_loss;       // v_r l(e_r) of every ray (may be NULL)
};

// The last argument of the DEPTH kernels: the regulariser's and the depth term's.  The other instantiations take RegArgs itself,
// so their argument block is what it was.
struct RegDepthArgs : RegArgs {
  DepthArgs z;
};
template <bool DEPTH>
using reg_args = std::conditional_t<DEPTH, RegDepthArgs, RegArgs>;

// the kernels' argument from the caller's struct; depth: an ACTIVE term, or NULL (all zero: nothing reads it)
inline DepthArgs make_depth_args(const rtxn_train_depth* depth, float loss_scale, int n_rays) {
  DepthArgs da{};
  if (depth) {
    da.weight = depth->weight;
    da.kind = depth->kind;
    da.param = depth->param;
    da.k = loss_scale * depth->weight / (float)n_rays;
    da.target = depth->target;
    da.depth = depth->depth;
    da.depth_loss = depth->depth_loss;
  }
  return da;
}

// k_z in a kernel: DepthArgs::k as the host formed it or (DEV) its expression in its order from the scale the wave read (reg_k's rule)
template <bool DEV>
__device__ __forceinline__ float depth_k(const DepthArgs& da, float loss_scale, int n_rays) {
  if constexpr (DEV) return loss_scale * da.weight / (float)n_rays;
  else return da.k;
}

// v_r l(e_r) and dl = v_r l'(e_r), e_r = D - z: a target is a finite z > 0 (0, negative, NaN, Inf: no target, both 0)
__device__ __forceinline__ float depth_term(const DepthArgs& da, float D, float z, float& dl) {
  dl = 0.0f;
  if (!(z > 0.0f && z <= 3.402823466e38f)) return 0.0f;
  return loss_term(da.kind, da.param, D, D - z, dl);
}

// a ray's share of the loss scalar: (lambda_z / n_rays) v_r l(e_r)
__device__ __forceinline__ float depth_loss_share(float weight, float l, float inv_rays) { return weight * l * inv_rays; }

}  // namespace
