// Ray gradients and camera pose refinement behind the hash-grid gather (include/rtxn.h, "ray gradients through the hash grid";
// DESIGN 5.16): the per-ray reduction of the segment end-point gradients, the per-image pose gradient, and the six-parameter Adam
// with the Rodrigues composition against the untouched poses.  tiny-cuda-nn exposes dL/dinput and instant-ngp builds its
// extrinsics optimisation on it; the reference has neither.  No atomics anywhere: every sum has a fixed order that does not depend
// on the launch, so the outputs are the same bits on every run.  Host-only sequencing plus three small kernels; nothing here reads
// the device on the host, so every call is hipGraph-capturable.
#include "common.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kRayLanes = 8;          // lanes per ray of the per-ray reduction

// d_origin[r] = sum_j (dstart_j + dend_j), d_direction[r] = sum_j (t_start_j dstart_j + t_end_j dend_j) over the ray's segments.
// Lane q of the ray's eight takes j = q, q + 8, ... in ascending order; the lanes are then summed by an xor butterfly (1, 2, 4).
__global__ __launch_bounds__(kThreads) void ray_gradients_kernel(const int* __restrict__ indices, const int* __restrict__ num_stored,
                                                                 const float* __restrict__ t_start, const float* __restrict__ t_end,
                                                                 const float* __restrict__ dstart, const float* __restrict__ dend, int n_rays,
                                                                 float* __restrict__ d_origin, float* __restrict__ d_direction) {
  const long tid = (long)blockIdx.x * kThreads + threadIdx.x;
  const long ray = tid / kRayLanes;
  const int q = (int)(tid % kRayLanes);
  const bool ok = ray < n_rays;                    // every lane stays: the butterfly reads across the eight
  const long first = ok ? indices[ray] : 0;
  const int n = ok ? num_stored[ray] : 0;
  float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = q; k < n; k += kRayLanes) {
    const long j = first + k;
    const float ts = t_start[j], te = t_end[j];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float ds = dstart[3 * j + a], de = dend[3 * j + a];
      acc[a] += ds + de;
      acc[3 + a] = fmaf(te, de, fmaf(ts, ds, acc[3 + a]));
    }
  }
#pragma unroll
  for (int m = 1; m < kRayLanes; m <<= 1)
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] += __shfl_xor(acc[c], m);
  if (ok && q == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      d_origin[3 * ray + a] = acc[a];
      d_direction[3 * ray + a] = acc[3 + a];
    }
  }
}

// One block per image: thread t sums its rays r = t, t + 256, ... in ascending order (those drawn from this image), then the
// block's 256 partial sums go through a fixed tree -- the wave's xor butterfly, then the four waves in order.
// grad[i] = (g_omega, g_tau, count, 0).
__global__ __launch_bounds__(kThreads) void pose_gradients_kernel(const uint32_t* __restrict__ drawn, const float* __restrict__ rays_d,
                                                                  const float* __restrict__ d_origin, const float* __restrict__ d_direction,
                                                                  int n_rays, float* __restrict__ grad) {
  __shared__ float part[kThreads / 64][7];
  const unsigned image = blockIdx.x;
  float acc[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int r = threadIdx.x; r < n_rays; r += kThreads) {
    if (drawn[2 * (long)r] != image) continue;
    const float d0 = rays_d[3 * (long)r], d1 = rays_d[3 * (long)r + 1], d2 = rays_d[3 * (long)r + 2];
    const float g0 = d_direction[3 * (long)r], g1 = d_direction[3 * (long)r + 1], g2 = d_direction[3 * (long)r + 2];
    acc[0] += fmaf(d1, g2, -(d2 * g1));            // d x dL/dd
    acc[1] += fmaf(d2, g0, -(d0 * g2));
    acc[2] += fmaf(d0, g1, -(d1 * g0));
#pragma unroll
    for (int a = 0; a < 3; ++a) acc[3 + a] += d_origin[3 * (long)r + a] / 10;      // make_ray: o = t / 10
    acc[6] += 1.0f;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1)
#pragma unroll
    for (int c = 0; c < 7; ++c) acc[c] += __shfl_xor(acc[c], m);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < 7; ++c) part[threadIdx.x >> 6][c] = acc[c];
  __syncthreads();
  if (threadIdx.x < 8) {
    float s = 0.0f;
    if (threadIdx.x < 7) {
      s = part[0][threadIdx.x];
      for (int w = 1; w < kThreads / 64; ++w) s += part[w][threadIdx.x];
    }
    grad[8 * (long)image + threadIdx.x] = s;
  }
}

// R(omega) of include/rtxn.h: I + A K + B K^2.  Below kTaylor the series of A and B through th^8; above, sin(th) / th and the
// half-angle form 2 sin^2(th / 2) / th^2, which loses nothing to cancellation where 1 - cos(th) would.
constexpr float kTaylor = 0.25f;
__device__ __forceinline__ void rodrigues(const float (&w)[3], float (&R)[9]) {
  const float t2 = fmaf(w[2], w[2], fmaf(w[1], w[1], w[0] * w[0]));
  const float th = sqrtf(t2);
  float A, B;
  if (th < kTaylor) {
    A = fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, 1.0f / 362880, -1.0f / 5040), 1.0f / 120), -1.0f / 6), 1.0f);
    B = fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, 1.0f / 3628800, -1.0f / 40320), 1.0f / 720), -1.0f / 24), 0.5f);
  } else {
    const float sh = sinf(0.5f * th);
    A = sinf(th) / th;
    B = 2.0f * (sh * sh) / t2;
  }
  const float xx = w[0] * w[0], yy = w[1] * w[1], zz = w[2] * w[2];
  const float xy = w[0] * w[1], xz = w[0] * w[2], yz = w[1] * w[2];
  R[0] = 1.0f - B * (yy + zz);
  R[4] = 1.0f - B * (xx + zz);
  R[8] = 1.0f - B * (xx + yy);
  R[1] = fmaf(B, xy, -(A * w[2]));
  R[3] = fmaf(B, xy, A * w[2]);
  R[2] = fmaf(B, xz, A * w[1]);
  R[6] = fmaf(B, xz, -(A * w[1]));
  R[5] = fmaf(B, yz, -(A * w[0]));
  R[7] = fmaf(B, yz, A * w[0]);
}

// poses[i] from delta[i] against poses0[i].  omega == 0 copies the rotation and a zero tau component copies the translation, so
// delta == 0 returns poses0 bit for bit (signed zeros included).
__device__ __forceinline__ void compose_pose(const float* __restrict__ p0, const float (&dl)[6], float* __restrict__ p) {
  const float w[3] = {dl[0], dl[1], dl[2]};
  if (w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) p[4 * r + c] = p0[4 * r + c];
  } else {
    float R[9];
    rodrigues(w, R);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) p[4 * r + c] = fmaf(R[3 * r + 2], p0[8 + c], fmaf(R[3 * r + 1], p0[4 + c], R[3 * r] * p0[c]));
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) p[4 * r + 3] = dl[3 + r] == 0.0f ? p0[4 * r + 3] : p0[4 * r + 3] + dl[3 + r];
#pragma unroll
  for (int c = 0; c < 4; ++c) p[12 + c] = p0[12 + c];
}

__global__ __launch_bounds__(64) void pose_step_kernel(rtxn_pose_refinement a, float one_minus_b1, float one_minus_b2) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_images) return;
  if (a.skip && *a.skip != 0u) return;                       // the optimizer skipped this step: every word keeps its bits
  const float* g = a.grad + 8 * (long)i;
  if (g[6] == 0.0f) return;                                  // not in the batch: moments and count stay (the table's sparse rule)
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) finite = finite && isfinite(g[c]);
  if (!finite) {
    if (a.skipped) atomicAdd(a.skipped, 1u);                 // an integer count: order-free
    return;
  }
  const int t = a.steps[i] + 1;
  a.steps[i] = t;
  // 1 - b^t in double, rounded once: rounding the power first leaves 2^-25 absolute on a difference of 1 - b2 = 1e-3 at t = 1, 2, ...
  const float c1 = (float)(1.0 - pow((double)a.beta1, (double)t)), c2 = (float)(1.0 - pow((double)a.beta2, (double)t));
  float dl[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const long e = 6 * (long)i + c;
    const float m = fmaf(a.beta1, a.m[e], one_minus_b1 * g[c]);
    const float v = fmaf(a.beta2, a.v[e], one_minus_b2 * (g[c] * g[c]));
    a.m[e] = m;
    a.v[e] = v;
    dl[c] = a.delta[e] - a.lr * ((m / c1) / (sqrtf(v / c2) + a.eps));
    a.delta[e] = dl[c];
  }
  compose_pose(a.poses0 + 16 * (long)i, dl, a.poses + 16 * (long)i);
}

// poses from delta alone, every image: what a loaded checkpoint or a reset calls
__global__ __launch_bounds__(64) void pose_compose_kernel(rtxn_pose_refinement a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_images) return;
  float dl[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) dl[c] = a.delta[6 * (long)i + c];
  compose_pose(a.poses0 + 16 * (long)i, dl, a.poses + 16 * (long)i);
}

}  // namespace

int rtxn::check_pose_refinement(const rtxn_pose_refinement* p, const char* who, bool need_buffers) {
  RTXN_REQUIRE(p, "%s: NULL pose refinement", who);
  RTXN_REQUIRE(p->n_images >= 1, "%s: pose->n_images = %d (>= 1)", who, p->n_images);
  RTXN_REQUIRE(std::isfinite(p->lr) && p->lr >= 0.0f, "%s: pose->lr = %g (finite, >= 0)", who, (double)p->lr);
  RTXN_REQUIRE(std::isfinite(p->beta1) && p->beta1 >= 0.0f && p->beta1 < 1.0f, "%s: pose->beta1 = %g (in [0, 1))", who, (double)p->beta1);
  RTXN_REQUIRE(std::isfinite(p->beta2) && p->beta2 >= 0.0f && p->beta2 < 1.0f, "%s: pose->beta2 = %g (in [0, 1))", who, (double)p->beta2);
  RTXN_REQUIRE(std::isfinite(p->eps) && p->eps > 0.0f, "%s: pose->eps = %g (finite, > 0)", who, (double)p->eps);
  if (need_buffers)
    RTXN_REQUIRE(p->poses0 && p->poses && p->delta && p->m && p->v && p->steps && p->grad,
                 "%s: pose: NULL among poses0 / poses / delta / m / v / steps / grad", who);
  return RTXN_OK;
}

extern "C" int rtxn_pose_refinement_check(const rtxn_pose_refinement* pose) {
  return rtxn::check_pose_refinement(pose, "rtxn_pose_refinement_check", false);
}

extern "C" int rtxn_ray_gradients_reduce(const int* indices, const int* num_stored, const float* t_start, const float* t_end,
                                         const float* dstart, const float* dend, int n_rays, float* d_origin, float* d_direction,
                                         rtxn_stream_t stream) {
  RTXN_REQUIRE(n_rays >= 0, "rtxn_ray_gradients_reduce: n_rays = %d < 0", n_rays);
  RTXN_DEVICE_OR_FAIL();
  if (n_rays == 0) return RTXN_OK;
  RTXN_REQUIRE(indices && num_stored && t_start && t_end && dstart && dend && d_origin && d_direction, "rtxn_ray_gradients_reduce: NULL buffer");
  const long threads = (long)n_rays * kRayLanes;
  ray_gradients_kernel<<<(unsigned)((threads + kThreads - 1) / kThreads), kThreads, 0, rtxn::as_stream(stream)>>>(
      indices, num_stored, t_start, t_end, dstart, dend, n_rays, d_origin, d_direction);
  RTXN_LAUNCH_CHECK("ray_gradients_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_pose_gradients(const uint32_t* drawn, const float* rays_d, const float* d_origin, const float* d_direction, int n_rays,
                                   const rtxn_pose_refinement* pose, rtxn_stream_t stream) {
  const int rc = rtxn::check_pose_refinement(pose, "rtxn_pose_gradients", true);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(n_rays >= 1, "rtxn_pose_gradients: n_rays = %d (>= 1)", n_rays);
  RTXN_REQUIRE(drawn && rays_d && d_origin && d_direction, "rtxn_pose_gradients: NULL among drawn / rays_d / d_origin / d_direction");
  RTXN_DEVICE_OR_FAIL();
  pose_gradients_kernel<<<(unsigned)pose->n_images, kThreads, 0, rtxn::as_stream(stream)>>>(drawn, rays_d, d_origin, d_direction, n_rays,
                                                                                            pose->grad);
  RTXN_LAUNCH_CHECK("pose_gradients_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_pose_step(const rtxn_pose_refinement* pose, rtxn_stream_t stream) {
  const int rc = rtxn::check_pose_refinement(pose, "rtxn_pose_step", true);
  if (rc != RTXN_OK) return rc;
  RTXN_DEVICE_OR_FAIL();
  pose_step_kernel<<<(unsigned)((pose->n_images + 63) / 64), 64, 0, rtxn::as_stream(stream)>>>(*pose, 1.0f - pose->beta1, 1.0f - pose->beta2);
  RTXN_LAUNCH_CHECK("pose_step_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_pose_compose(const rtxn_pose_refinement* pose, rtxn_stream_t stream) {
  const int rc = rtxn::check_pose_refinement(pose, "rtxn_pose_compose", true);
  if (rc != RTXN_OK) return rc;
  RTXN_DEVICE_OR_FAIL();
  pose_compose_kernel<<<(unsigned)((pose->n_images + 63) / 64), 64, 0, rtxn::as_stream(stream)>>>(*pose);
  RTXN_LAUNCH_CHECK("pose_compose_kernel");
  return RTXN_OK;
}
