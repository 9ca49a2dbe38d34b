// The element update shared by every Adam kernel of the library (train.hip: adam_kernel, adam_sparse_kernel; optimizer.hip: their
// forms under rtxn_optimizer_options).
#pragma once
#include <hip/hip_runtime.h>

// One Adam update (tcnn "Adam": no weight decay, bias correction folded into lr_eff on the host / lr_dev).
__device__ __forceinline__ void adam_one(float g, float& mi, float& vi, float& w, float lr_eff, float beta1, float beta2, float eps) {
  mi = beta1 * mi + (1.0f - beta1) * g;
  vi = beta2 * vi + (1.0f - beta2) * g * g;
  w = w - lr_eff * mi / (sqrtf(vi) + eps);
}
