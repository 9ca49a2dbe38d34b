// Intrinsics refinement (include/rtxn.h, rtxn_camera_refinement): the gradient of a drawn ray's direction with
// respect to its camera row -- through the two lens models' Newton solves by the implicit function theorem, at the solution the
// draw itself computed (camera_internal.h's own functions) -- its per-camera sum, and the three-group Adam that rewrites the
// live rows against an untouched copy.  instant-ngp optimises intrinsics beside extrinsics; the reference has neither.  No
// atomics on a float anywhere: every sum has a fixed order that does not depend on the launch or on n_rays' alignment.  Host-only
// sequencing plus four small kernels; nothing here reads the device on the host, so every call is hipGraph-capturable.
#include "common.h"
#include "camera_internal.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kTerms = 12;            // floats per ray of scratch and per camera of grad: ten sums, the count, one pad
constexpr int kDelta = 10;            // fx, fy, cx, cy, k1, k2, k3, k4, p1, p2

// bit e: the model has parameter e (k4 is the fisheye's alone, p1 and p2 the radial-tangential model's)
__host__ __device__ constexpr unsigned model_mask(int model) {
  return model == RTXN_CAMERA_OPENCV ? 0x37Fu : model == RTXN_CAMERA_OPENCV_FISHEYE ? 0x0FFu : 0x00Fu;
}

// One thread per ray: terms[r] = dL/d(fx, fy, cx, cy, k1, k2, k3, k4, p1, p2) of ray r alone, then two zeros.
template <int MODEL>
__global__ __launch_bounds__(kThreads) void camera_terms_kernel(const uint32_t* __restrict__ drawn, const float* __restrict__ d_direction,
                                                                int n_rays, const float* __restrict__ poses, const float* __restrict__ params,
                                                                int n_cameras, unsigned width, float* __restrict__ terms) {
  const long r = (long)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n_rays) return;   // tail block
  const unsigned image = drawn[2 * r], pixel = drawn[2 * r + 1];
  if (n_cameras != 1 && image >= (unsigned)n_cameras) return;   // no such camera: the fold never selects this ray
  const float* cam = params + (size_t)RTXN_CAMERA_PARAMS * (n_cameras == 1 ? 0u : image);
  const float* la = poses + 16 * (size_t)image;
  const float fx = cam[0], fy = cam[1];
  // camera_ray's own expressions: the point of linearisation is the ray that was drawn
  const float xd = ((float)(pixel % width) + 0.5f - cam[2]) / fx;
  const float yd = ((float)(pixel / width) + 0.5f - cam[3]) / fy;
  float q0 = xd, q1 = yd, q2 = -1.0f, thd = 0.0f, th = 0.0f;
  bool lens = MODEL == RTXN_CAMERA_OPENCV;
  if (MODEL == RTXN_CAMERA_OPENCV) {
    rtxn::undistort_opencv(cam, xd, yd, q0, q1);
  } else if (MODEL == RTXN_CAMERA_OPENCV_FISHEYE) {
    thd = sqrtf(fmaf(xd, xd, yd * yd));
    lens = thd >= 1e-8f;
    if (lens) {
      th = rtxn::undistort_fisheye(cam, thd);
      const float s = sinf(th) / thd;
      q0 = s * xd;
      q1 = s * yd;
      q2 = -cosf(th);
    }
  }
  const float w0 = fmaf(la[2], q2, fmaf(la[0], q0, la[1] * q1));
  const float w1 = fmaf(la[6], q2, fmaf(la[4], q0, la[5] * q1));
  const float w2 = fmaf(la[10], q2, fmaf(la[8], q0, la[9] * q1));
  const float norm = sqrtf(fmaf(w2, w2, fmaf(w0, w0, w1 * w1)));
  const float d0 = w0 / norm, d1 = w1 / norm, d2 = w2 / norm;
  const float g0 = d_direction[3 * r], g1 = d_direction[3 * r + 1], g2 = d_direction[3 * r + 2];
  // through the normalisation, then R^T
  const float gd = fmaf(g2, d2, fmaf(g0, d0, g1 * d1));
  const float gw0 = fmaf(-d0, gd, g0) / norm, gw1 = fmaf(-d1, gd, g1) / norm, gw2 = fmaf(-d2, gd, g2) / norm;
  const float gq0 = fmaf(la[8], gw2, fmaf(la[0], gw0, la[4] * gw1));
  const float gq1 = fmaf(la[9], gw2, fmaf(la[1], gw0, la[5] * gw1));
  const float gq2 = fmaf(la[10], gw2, fmaf(la[2], gw0, la[6] * gw1));
  float lx = gq0, ly = gq1;                       // dL/d(xd, yd): the pinhole's, and the fisheye's at the principal point
  float t[kTerms] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (MODEL == RTXN_CAMERA_OPENCV) {
    // F(x, y; k) = (xd, yd):  d(x, y)/d(xd, yd) = J^-1,  d(x, y)/dk = -J^-1 dF/dk,  J symmetric
    float f0, f1, j11, j12, j22;
    rtxn::opencv_forward(cam, q0, q1, f0, f1, j11, j12, j22);
    const float det = fmaf(j11, j22, -(j12 * j12));
    lx = fmaf(j22, gq0, -(j12 * gq1)) / det;
    ly = fmaf(j11, gq1, -(j12 * gq0)) / det;
    const float xx = q0 * q0, yy = q1 * q1, xy2 = 2.0f * (q0 * q1);
    const float r2 = xx + yy;
    const float rl = -fmaf(lx, q0, ly * q1);
    t[4] = rl * r2;
    t[5] = rl * (r2 * r2);
    t[6] = rl * (r2 * r2 * r2);
    t[8] = -fmaf(lx, xy2, ly * fmaf(2.0f, yy, r2));
    t[9] = -fmaf(lx, fmaf(2.0f, xx, r2), ly * xy2);
  } else if (MODEL == RTXN_CAMERA_OPENCV_FISHEYE) {
    if (lens) {
      // q = (sin(th) u, -cos(th)), u = (xd, yd) / thd, th(thd; k) from thd = th poly(th)
      const float ux = xd / thd, uy = yd / thd;
      const float sn = sinf(th), cs = cosf(th);
      const float dpoly = rtxn::fisheye_dpoly(cam, th);
      const float gth = fmaf(sn, gq2, cs * fmaf(gq0, ux, gq1 * uy));
      const float a0 = sn * gq0, a1 = sn * gq1;
      const float au = fmaf(a0, ux, a1 * uy);
      const float gr = gth / dpoly;
      lx = fmaf(gr, ux, fmaf(-au, ux, a0) / thd);
      ly = fmaf(gr, uy, fmaf(-au, uy, a1) / thd);
      const float t2 = th * th;
      float p = th * t2;                          // th^(2n+1)
      t[4] = -gr * p;
      p *= t2;
      t[5] = -gr * p;
      p *= t2;
      t[6] = -gr * p;
      p *= t2;
      t[7] = -gr * p;
    }
  }
  t[0] = -(lx * xd) / fx;
  t[1] = -(ly * yd) / fy;
  t[2] = -lx / fx;
  t[3] = -ly / fy;
  float4* out = reinterpret_cast<float4*>(terms + kTerms * r);
  out[0] = make_float4(t[0], t[1], t[2], t[3]);
  out[1] = make_float4(t[4], t[5], t[6], t[7]);
  out[2] = make_float4(t[8], t[9], 0.0f, 0.0f);
}

// One block per camera, pose_gradients_kernel's fold: thread t sums its rays r = t, t + 256, ... in ascending order (those of
// this camera; every ray for a shared camera), then the wave's xor butterfly, then the four waves in order.
// grad[c] = (ten sums, count, 0).
__global__ __launch_bounds__(kThreads) void camera_fold_kernel(const uint32_t* __restrict__ drawn, const float* __restrict__ terms, int n_rays,
                                                               int n_cameras, float* __restrict__ grad) {
  __shared__ float part[kThreads / 64][kDelta + 1];
  const unsigned camera = blockIdx.x;
  float acc[kDelta + 1];
#pragma unroll
  for (int c = 0; c <= kDelta; ++c) acc[c] = 0.0f;
  for (int r = threadIdx.x; r < n_rays; r += kThreads) {
    if (n_cameras != 1 && drawn[2 * (long)r] != camera) continue;
    const float4* src = reinterpret_cast<const float4*>(terms + kTerms * (long)r);
    const float4 a = src[0], b = src[1], c = src[2];
    acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
    acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
    acc[8] += c.x; acc[9] += c.y;
    acc[10] += 1.0f;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1)
#pragma unroll
    for (int c = 0; c <= kDelta; ++c) acc[c] += __shfl_xor(acc[c], m);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c <= kDelta; ++c) part[threadIdx.x >> 6][c] = acc[c];
  __syncthreads();
  if (threadIdx.x < kTerms) {
    float s = 0.0f;
    if (threadIdx.x <= kDelta) {
      s = part[0][threadIdx.x];
      for (int w = 1; w < kThreads / 64; ++w) s += part[w][threadIdx.x];
    }
    grad[kTerms * (long)camera + threadIdx.x] = s;
  }
}

// Entry e of the row from delta against params0.  delta == 0 copies the loaded word, so a zero delta returns params0 bit for bit.
__device__ __forceinline__ float compose_entry(int e, float p0, float dl) {
  if (dl == 0.0f) return p0;
  return e < 2 ? p0 * expf(dl) : p0 + dl;
}

__global__ __launch_bounds__(64) void camera_step_kernel(rtxn_camera_refinement a, float one_minus_b1, float one_minus_b2) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_cameras) return;
  if (a.skip && *a.skip != 0u) return;                       // the optimizer skipped this step: every word keeps its bits
  const float* g = a.grad + kTerms * (long)i;
  if (g[kDelta] == 0.0f) return;                             // not in the batch: moments and count stay (the table's sparse rule)
  const unsigned has = model_mask(a.model);
  const float* p0 = a.params0 + (long)RTXN_CAMERA_PARAMS * i;
  float* p = a.params + (long)RTXN_CAMERA_PARAMS * i;
  float gd[kDelta], lr[kDelta], bound[kDelta];
  unsigned active = 0u;
  bool finite = true;
#pragma unroll
  for (int e = 0; e < kDelta; ++e) {
    lr[e] = e < 2 ? a.lr_focal : e < 4 ? a.lr_center : a.lr_distortion;
    bound[e] = e < 2 ? a.max_log_focal : e < 4 ? a.max_center : a.max_distortion;
    gd[e] = e < 2 ? g[e] * p[e] : g[e];                      // fx = fx0 exp(delta): d/d(delta) = dL/dfx fx
    if (((has >> e) & 1u) && lr[e] > 0.0f) {
      active |= 1u << e;
      finite = finite && isfinite(gd[e]);
    }
  }
  if (active == 0u) return;                                  // every group frozen
  if (!finite) {
    if (a.skipped) atomicAdd(a.skipped, 1u);                 // an integer count: order-free
    return;
  }
  const int t = a.steps[i] + 1;
  a.steps[i] = t;
  // 1 - b^t in double, rounded once, as pose_step_kernel forms it
  const float c1 = (float)(1.0 - pow((double)a.beta1, (double)t)), c2 = (float)(1.0 - pow((double)a.beta2, (double)t));
#pragma unroll
  for (int e = 0; e < kDelta; ++e) {
    if (!((active >> e) & 1u)) continue;                     // a frozen group, an entry the model lacks: no word is written
    const long k = kDelta * (long)i + e;
    const float m = fmaf(a.beta1, a.m[k], one_minus_b1 * gd[e]);
    const float v = fmaf(a.beta2, a.v[k], one_minus_b2 * (gd[e] * gd[e]));
    a.m[k] = m;
    a.v[k] = v;
    float dl = a.delta[k] - lr[e] * ((m / c1) / (sqrtf(v / c2) + a.eps));
    dl = fminf(fmaxf(dl, -bound[e]), bound[e]);
    a.delta[k] = dl;
    p[e] = compose_entry(e, p0[e], dl);
  }
}

// rows from delta alone, every camera and all twelve words: what a loaded checkpoint or a reset calls
__global__ __launch_bounds__(64) void camera_compose_kernel(rtxn_camera_refinement a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_cameras) return;
  const unsigned has = model_mask(a.model);
  const float* p0 = a.params0 + (long)RTXN_CAMERA_PARAMS * i;
  float* p = a.params + (long)RTXN_CAMERA_PARAMS * i;
#pragma unroll
  for (int e = 0; e < RTXN_CAMERA_PARAMS; ++e)
    p[e] = e < kDelta && ((has >> e) & 1u) ? compose_entry(e, p0[e], a.delta[kDelta * (long)i + e]) : p0[e];
}

}  // namespace

int rtxn::check_camera_refinement(const rtxn_camera_refinement* c, const char* who, bool need_buffers) {
  RTXN_REQUIRE(c, "%s: NULL camera refinement", who);
  RTXN_REQUIRE(c->model == RTXN_CAMERA_PINHOLE || c->model == RTXN_CAMERA_OPENCV || c->model == RTXN_CAMERA_OPENCV_FISHEYE,
               "%s: cameras->model = %d: unknown camera model", who, c->model);
  RTXN_REQUIRE(c->n_cameras >= 1, "%s: cameras->n_cameras = %d (>= 1)", who, c->n_cameras);
  const struct { const char* name; float v; } rates[] = {{"lr_focal", c->lr_focal}, {"lr_center", c->lr_center}, {"lr_distortion", c->lr_distortion}};
  for (const auto& r : rates)
    RTXN_REQUIRE(std::isfinite(r.v) && r.v >= 0.0f, "%s: cameras->%s = %g (finite, >= 0)", who, r.name, (double)r.v);
  const struct { const char* name; float v; } bounds[] = {{"max_log_focal", c->max_log_focal}, {"max_center", c->max_center},
                                                          {"max_distortion", c->max_distortion}};
  for (const auto& b : bounds) RTXN_REQUIRE(b.v >= 0.0f, "%s: cameras->%s = %g (>= 0)", who, b.name, (double)b.v);
  RTXN_REQUIRE(std::isfinite(c->beta1) && c->beta1 >= 0.0f && c->beta1 < 1.0f, "%s: cameras->beta1 = %g (in [0, 1))", who, (double)c->beta1);
  RTXN_REQUIRE(std::isfinite(c->beta2) && c->beta2 >= 0.0f && c->beta2 < 1.0f, "%s: cameras->beta2 = %g (in [0, 1))", who, (double)c->beta2);
  RTXN_REQUIRE(std::isfinite(c->eps) && c->eps > 0.0f, "%s: cameras->eps = %g (finite, > 0)", who, (double)c->eps);
  if (need_buffers) {
    RTXN_REQUIRE(c->params0 && c->params && c->delta && c->m && c->v && c->steps && c->grad,
                 "%s: cameras: NULL among params0 / params / delta / m / v / steps / grad", who);
  }
  return RTXN_OK;
}

extern "C" int rtxn_camera_refinement_check(const rtxn_camera_refinement* cameras) {
  return rtxn::check_camera_refinement(cameras, "rtxn_camera_refinement_check", false);
}

extern "C" int rtxn_camera_gradients(const uint32_t* drawn, const float* d_direction, int n_rays, const float* set_poses,
                                     const rtxn_camera_refinement* cameras, rtxn_stream_t stream) {
  const char* who = "rtxn_camera_gradients";
  const int rc = rtxn::check_camera_refinement(cameras, who, true);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(n_rays >= 1, "%s: n_rays = %d (>= 1)", who, n_rays);
  RTXN_REQUIRE(drawn && d_direction && set_poses, "%s: NULL among drawn / d_direction / set_poses", who);
  RTXN_REQUIRE(cameras->terms && cameras->width >= 1, "%s: cameras->terms = %p, cameras->width = %u: the per-ray scratch and the frame's width",
               who, (void*)cameras->terms, cameras->width);
  RTXN_REQUIRE(((uintptr_t)cameras->terms & 15u) == 0, "%s: cameras->terms must be 16-byte aligned", who);
  RTXN_DEVICE_OR_FAIL();
  hipStream_t st = rtxn::as_stream(stream);
  const dim3 grid(((unsigned)n_rays + kThreads - 1) / kThreads), block(kThreads);
  const rtxn_camera_refinement& c = *cameras;
  switch (c.model) {
    case RTXN_CAMERA_PINHOLE:
      camera_terms_kernel<RTXN_CAMERA_PINHOLE><<<grid, block, 0, st>>>(drawn, d_direction, n_rays, set_poses, c.params, c.n_cameras, c.width, c.terms);
      break;
    case RTXN_CAMERA_OPENCV:
      camera_terms_kernel<RTXN_CAMERA_OPENCV><<<grid, block, 0, st>>>(drawn, d_direction, n_rays, set_poses, c.params, c.n_cameras, c.width, c.terms);
      break;
    default:
      camera_terms_kernel<RTXN_CAMERA_OPENCV_FISHEYE><<<grid, block, 0, st>>>(drawn, d_direction, n_rays, set_poses, c.params, c.n_cameras, c.width,
                                                                              c.terms);
      break;
  }
  RTXN_LAUNCH_CHECK("camera_terms_kernel");
  camera_fold_kernel<<<(unsigned)c.n_cameras, kThreads, 0, st>>>(drawn, c.terms, n_rays, c.n_cameras, c.grad);
  RTXN_LAUNCH_CHECK("camera_fold_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_camera_step(const rtxn_camera_refinement* cameras, rtxn_stream_t stream) {
  const int rc = rtxn::check_camera_refinement(cameras, "rtxn_camera_step", true);
  if (rc != RTXN_OK) return rc;
  RTXN_DEVICE_OR_FAIL();
  camera_step_kernel<<<(unsigned)((cameras->n_cameras + 63) / 64), 64, 0, rtxn::as_stream(stream)>>>(*cameras, 1.0f - cameras->beta1,
                                                                                                     1.0f - cameras->beta2);
  RTXN_LAUNCH_CHECK("camera_step_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_camera_compose(const rtxn_camera_refinement* cameras, rtxn_stream_t stream) {
  const int rc = rtxn::check_camera_refinement(cameras, "rtxn_camera_compose", true);
  if (rc != RTXN_OK) return rc;
  RTXN_DEVICE_OR_FAIL();
  camera_compose_kernel<<<(unsigned)((cameras->n_cameras + 63) / 64), 64, 0, rtxn::as_stream(stream)>>>(*cameras);
  RTXN_LAUNCH_CHECK("camera_compose_kernel");
  return RTXN_OK;
}
