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
// Also here: the same fixed-order sum and the stand-alone elementwise kernel (rtxn_loss) for the losses of rtxn_train_loss.
#include "background_internal.h"
#include "common.h"
#include "depth_internal.h"
#include "loss_internal.h"
#include "reg_internal.h"

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

// The same sum for the losses of rtxn_train_loss (composite_train.hip's kernels; include/rtxn.h): the per-ray term is
// loss_internal.h's ray_loss_term, the function the compositor evaluates, on the pixels it stored and -- with lambda > 0 -- on
// the opacities it stored; grouping and order are l2_loss_fixed_order_kernel's.  REG: the regulariser's share is added per ray
// from the L_r the compositor stored, by the expression the compositor itself adds (reg_internal.h).  DEPTH: likewise the depth
// term's share, from the D_r the compositor stored and the ray's target (depth_internal.h).
template <bool REG, bool DEPTH>
__global__ __launch_bounds__(kLossThreads) void loss_fixed_order_kernel(const float* __restrict__ pixels, const float* __restrict__ target,
                                                                        int n_rays, BgArgs bg, LossArgs la, float* __restrict__ loss_sum,
                                                                        RegArgs ra, DepthArgs da) {
  __shared__ float red[kLossThreads];
  const float inv_n = 1.0f / (float)(3L * n_rays), inv_rays = 1.0f / (float)n_rays;
  const int groups = (n_rays + 3) / 4;
  float acc = 0.0f;
  for (int g = threadIdx.x; g < groups; g += kLossThreads) {
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ray = 4 * g + k;
      e[k] = 0.0f;
      if (ray < n_rays) {
        float b[3], t[3], dl[3], dA;
        ray_background(bg, target, ray, b, t);
        const float p[3] = {pixels[3 * (long)ray], pixels[3 * (long)ray + 1], pixels[3 * (long)ray + 2]};
        const bool alpha_term = la.opacity_weight > 0.0f;
        e[k] = ray_loss_term(la, p, t, alpha_term ? la.opacity[ray] : 0.0f, alpha_term ? target[4 * (long)ray + 3] : 0.0f, inv_n, inv_rays,
                             dl, dA);
        if constexpr (REG) {
          if (ra.weight > 0.0f) e[k] += reg_loss_share(ra.weight, ra.distortion[ray], inv_rays);
        }
        if constexpr (DEPTH) {
          if (da.weight > 0.0f) {
            float dlz;
            e[k] += depth_loss_share(da.weight, depth_term(da, da.depth[ray], da.target[ray], dlz), inv_rays);
          }
        }
      }
    }
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

// rtxn_loss: loss->evaluate for the four kinds, elementwise (l2_loss_kernel's role, train.hip), N = n
constexpr int kElemThreads = 256;
__global__ __launch_bounds__(kElemThreads) void loss_kernel(const float* __restrict__ pred, const float* __restrict__ target, long n,
                                                            float scale, int kind, float param, float* __restrict__ values,
                                                            __half* __restrict__ grads, float* __restrict__ loss_sum) {
  __shared__ float red[kElemThreads / 64];
  const float inv_n = 1.0f / (float)n;
  float local = 0.0f;
  for (long i = (long)blockIdx.x * kElemThreads + threadIdx.x; i < n; i += (long)gridDim.x * kElemThreads) {
    const float p = pred[i];
    float dl;
    const float v = loss_term(kind, param, p, p - target[i], dl) * inv_n;
    if (values) values[i] = v;
    if (grads) grads[i] = loss_grad_half(scale, dl, inv_n);
    local += v;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) local += __shfl_xor(local, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0 && loss_sum) {
    float t = 0.0f;
    for (int w = 0; w < kElemThreads / 64; ++w) t += red[w];
    atomicAdd(loss_sum, t);
  }
}

}  // namespace

namespace rtxn {

int loss_fixed_order(const float* pixels, const float* target, int n_rays, const rtxn_train_background* bg, const rtxn_train_loss* loss,
                     const rtxn_train_regularizer* reg, const rtxn_train_depth* depth, float* loss_sum, hipStream_t stream) {
  const BgArgs a = make_bg_args(bg);
  const LossArgs la = make_loss_args(loss, bg != nullptr);
  const RegArgs ra = make_reg_args(reg, 1.0f, n_rays);      // the loss scale enters sweep 2's factor only: not read here
  const DepthArgs da = make_depth_args(depth, 1.0f, n_rays);
  auto* const kernel = depth ? (reg ? loss_fixed_order_kernel<true, true> : loss_fixed_order_kernel<false, true>)
                             : (reg ? loss_fixed_order_kernel<true, false> : loss_fixed_order_kernel<false, false>);
  kernel<<<1, kLossThreads, 0, stream>>>(pixels, target, n_rays, a, la, loss_sum, ra, da);
  RTXN_LAUNCH_CHECK("loss_fixed_order_kernel");
  return RTXN_OK;
}

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

extern "C" int rtxn_loss(const float* pred, const float* target, long n, const rtxn_train_loss* loss, float loss_scale, float* values,
                         void* grads_half, float* loss_sum, rtxn_stream_t stream) {
  bool active = false;
  const int rc = rtxn::check_train_loss(loss, 3, -1, "rtxn_loss", &active);
  if (rc != RTXN_OK) return rc;
  if (!active) return rtxn_l2_loss(pred, target, n, loss_scale, values, grads_half, loss_sum, stream);      // NULL or L2: the L2 kernel itself
  RTXN_REQUIRE(n >= 0, "rtxn_loss: n = %ld < 0", n);
  RTXN_DEVICE_OR_FAIL();
  hipStream_t s = rtxn::as_stream(stream);
  if (loss_sum) RTXN_HIP(rtxn::zero_words(loss_sum, 1, s));
  if (n == 0) return RTXN_OK;
  RTXN_REQUIRE(pred && target, "rtxn_loss: NULL buffer");
  const long want = (n + kElemThreads - 1) / kElemThreads;
  loss_kernel<<<(unsigned)(want < 1024 ? want : 1024), kElemThreads, 0, s>>>(pred, target, n, loss_scale, loss->kind, loss->param, values,
                                                                             static_cast<__half*>(grads_half), loss_sum);
  RTXN_LAUNCH_CHECK("loss_kernel");
  return RTXN_OK;
}
