// The L2 loss SCALAR of a training batch in deterministic mode (rtxn_set_deterministic_workspace).  The training compositor
// (volrender.hip, volrender_l2_*_kernel) adds its loss with float atomics -- one per block of four rays in the *_multi_kernel<4>
// forms, one per ray in the one-ray-per-wave forms for odd K or misaligned buffers -- so the scalar's last bit follows the order
// the blocks retire in.  Deterministic mode promises two runs of the same steps identical bits, and the scalar is what a step
// returns: with a workspace registered the compositor is launched WITHOUT a loss pointer and this kernel forms the sum behind
// it from what the compositor left -- pixels and targets -- in ONE fixed order, whichever compositor form ran.  The per-ray
// term is the compositor's own, operation for operation (-ffp-contract=off on both sides):
//   ray r:    e_r = (d0^2 + d1^2 + d2^2) * (1 / (3 n_rays)),  d_c = pixels[r][c] - t_c, t the ray's target -- straight RGBA
//             targets composited over the ray's background by the compositor's own ray_background (background_internal.h);
//   group g:  (e_4g + e_4g+1) + (e_4g+2 + e_4g+3), rays past the batch counting 0 (the grouping of the four-ray blocks; for the
//             per-ray forms it is simply this kernel's order);
//   total:    thread t of 1024 adds groups t, t + 1024, ... in ascending order, then a shared-memory tree over the threads.
// The value differs from the atomics' sum by float rounding of the order only (tests/test_gpu_deterministic_loss.py holds it
// to a float64 restatement from pixels and targets).  One block: a 4096-ray batch is one group per thread.  Default mode
// never comes here.
#include "background_internal.h"
#include "common.h"

namespace {

constexpr int kLossThreads = 1024;

__device__ __forceinline__ float ray_loss(const float* __restrict__ pixels, const float* __restrict__ target, int ray, float inv_n,
                                          const BgArgs& bg) {
  float b[3], t[3];
  ray_background(bg, target, ray, b, t);
  const float d0 = pixels[3 * (long)ray] - t[0], d1 = pixels[3 * (long)ray + 1] - t[1], d2 = pixels[3 * (long)ray + 2] - t[2];
  return (d0 * d0 + d1 * d1 + d2 * d2) * inv_n;
}

__global__ __launch_bounds__(kLossThreads) void l2_loss_fixed_order_kernel(const float* __restrict__ pixels,
                                                                           const float* __restrict__ target, int n_rays, BgArgs bg,
                                                                           float* __restrict__ loss_sum) {
  __shared__ float red[kLossThreads];
  const float inv_n = 1.0f / (float)(3L * n_rays);
  const int groups = (n_rays + 3) / 4;
  float acc = 0.0f;
  for (int g = threadIdx.x; g < groups; g += kLossThreads) {
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = 4 * g + k < n_rays ? ray_loss(pixels, target, 4 * g + k, inv_n, bg) : 0.0f;
    acc += (e[0] + e[1]) + (e[2] + e[3]);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kLossThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss_sum = red[0];
}

}  // namespace

namespace rtxn {

int l2_loss_fixed_order(const float* pixels, const float* target, int n_rays, int bg_mode, const float* bg_color, unsigned bg_seed,
                        const int* bg_step, int target_channels, float* loss_sum, hipStream_t stream) {
  BgArgs bg{};
  bg.mode = bg_mode;
  for (int c = 0; c < 3; ++c) bg.color[c] = bg_color ? bg_color[c] : 0.0f;
  bg.seed = bg_seed;
  bg.step = bg_step;
  bg.target_channels = target_channels;
  l2_loss_fixed_order_kernel<<<1, kLossThreads, 0, stream>>>(pixels, target, n_rays, bg, loss_sum);
  RTXN_LAUNCH_CHECK("l2_loss_fixed_order_kernel");
  return RTXN_OK;
}

}  // namespace rtxn
