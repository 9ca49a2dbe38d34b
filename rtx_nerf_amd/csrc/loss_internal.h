// The training losses of rtxn_train_loss (include/rtxn.h): the per-channel term l(e) with its derivative dl/dp,
// and the per-ray alpha term, shared by the loss compositor (composite_train.hip), the fixed-order loss sum and the stand-alone
// loss kernel (loss.hip) so that all three form a scalar from the same operations, bit for bit (-ffp-contract=off on every
// side).  Internal to librtxn.so.  The struct stays in an anonymous namespace, as BgArgs does: kernels take it by value.
#pragma once
#include "common.h"

namespace {

struct LossArgs {
  int kind;               // rtxn_loss_kind
  float param;            // HUBER: delta; RELATIVE_L2: epsilon
  float opacity_weight;   // lambda
  int has_background;     // the compositor adds (1 - A) b to the pixel
  float* opacity;         // compositor: A of every ray is written here (may be NULL); the loss sums read it when lambda > 0
};

// the kernels' argument from the caller's struct; loss: an ACTIVE loss, or NULL for L2 with no alpha term and no opacity output
inline LossArgs make_loss_args(const rtxn_train_loss* loss, bool has_background) {
  LossArgs la{};
  la.kind = RTXN_LOSS_L2;
  if (loss) {
    la.kind = loss->kind;
    la.param = loss->param;
    la.opacity_weight = loss->opacity_weight;
    la.opacity = loss->opacity;
  }
  la.has_background = has_background ? 1 : 0;
  return la;
}

// l(e) of one channel, e = p - t; dl = dl/dp (relative L2: the denominator is a constant to the gradient; IEEE division)
__device__ __forceinline__ float loss_term(int kind, float param, float p, float e, float& dl) {
  if (kind == RTXN_LOSS_L1) {
    dl = e > 0.0f ? 1.0f : e < 0.0f ? -1.0f : 0.0f;
    return fabsf(e);
  }
  if (kind == RTXN_LOSS_HUBER) {
    const float a = fabsf(e);
    dl = fminf(fmaxf(e, -param), param);
    return a <= param ? 0.5f * e * e : param * (a - 0.5f * param);
  }
  if (kind == RTXN_LOSS_RELATIVE_L2) {
    const float den = p * p + param;
    dl = 2.0f * e / den;
    return e * e / den;
  }
  dl = 2.0f * e;
  return e * e;
}

// One ray's share of the loss scalar: (l_0 + l_1 + l_2) / N + (lambda / n_rays) (A - alpha)^2 (the second part only when
// lambda > 0), and the derivatives the compositor rounds to fp16: dl[c] = dl/dp_c, dA = 2 (A - alpha).
__device__ __forceinline__ float ray_loss_term(const LossArgs& la, const float (&p)[3], const float (&t)[3], float A, float alpha,
                                               float inv_n, float inv_rays, float (&dl)[3], float& dA) {
  float l[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) l[c] = loss_term(la.kind, la.param, p[c], p[c] - t[c], dl[c]);
  float v = (l[0] + l[1] + l[2]) * inv_n;
  dA = 0.0f;
  if (la.opacity_weight > 0.0f) {
    const float d = A - alpha;
    dA = 2.0f * d;
    v += la.opacity_weight * (d * d) * inv_rays;
  }
  return v;
}

// the fp16 gradients handed on: g_c = half(loss_scale l'(e_c) / N), g_A = half(loss_scale lambda 2 (A - alpha) / n_rays)
__device__ __forceinline__ __half loss_grad_half(float loss_scale, float dl, float inv_n) { return __float2half(loss_scale * dl * inv_n); }
__device__ __forceinline__ __half opacity_grad_half(float loss_scale, float lambda, float dA, float inv_rays) {
  return __float2half(loss_scale * (lambda * dA) * inv_rays);
}

}  // namespace
