// Depth targets of a drawn batch (rtxn_depth_targets, include/rtxn.h): the resident depth maps stay as loaded
// (16-bit integers in the file's unit, or floats), and one thread per ray turns the drawn pixel's value into the distance along
// the ray that the compositor's D_r = sum w m is compared with.  A z-depth map (the usual kind: distance along the optical axis)
// is divided by the cosine between the ray and the axis, taken from the ray itself and the LIVE pose, so every camera model and
// a refined pose are honoured without this kernel knowing either.
//
// A gather like the draw: per ray 8 B of drawn, 12 B of direction, 12 B of one pose column (n_images of them, L2-resident) and
// one 2- or 4-byte map value read, 4 B written -- launch latency, not bandwidth.
#include <cmath>

#include "common.h"

namespace {

template <bool U16>
__global__ __launch_bounds__(256) void depth_targets_kernel(rtxn_depth_targets_args a) {
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  if (r >= (unsigned)a.n_rays) return;   // tail block
  const unsigned image = a.drawn[2 * (size_t)r], pixel = a.drawn[2 * (size_t)r + 1];
  const unsigned n_pixels = a.width * a.height;   // <= 1 << 24 (checked by the entry point)
  float out = 0.0f;
  if (image < (unsigned)a.n_images && pixel < n_pixels) {      // anything else is not a pixel of the set: no target, nothing read
    const size_t texel = (size_t)image * n_pixels + pixel;
    const float v = U16 ? (float)static_cast<const uint16_t*>(a.depth)[texel] : static_cast<const float*>(a.depth)[texel];
    if (v > 0.0f && v <= 3.402823466e38f) {                    // 0, negative, NaN, Inf: no target
      const float t = v * a.scale;
      if (a.kind == RTXN_DEPTH_RAY) {
        out = t;
      } else {
        const float* __restrict__ la = a.poses + 16 * (size_t)image;
        const float l0 = la[2], l1 = la[6], l2 = la[10];
        const float d0 = a.rays_d[3 * (size_t)r], d1 = a.rays_d[3 * (size_t)r + 1], d2 = a.rays_d[3 * (size_t)r + 2];
        const float c = -(d0 * l0 + d1 * l1 + d2 * l2) / sqrtf(l0 * l0 + l1 * l1 + l2 * l2);
        if (c > 0x1p-6f) out = t / c;                          // a grazing ray (or NaN): no target
      }
    }
  }
  a.target[r] = out;
}

}  // namespace

extern "C" int rtxn_depth_targets(const rtxn_depth_targets_args* a, rtxn_stream_t stream) {
  const char* who = "rtxn_depth_targets";
  RTXN_REQUIRE(a != nullptr, "%s: args is NULL", who);
  RTXN_REQUIRE(a->depth && a->poses, "%s: NULL depth or poses", who);
  RTXN_REQUIRE(a->drawn && a->rays_d && a->target, "%s: NULL drawn, rays_d or target", who);
  RTXN_REQUIRE(a->format == RTXN_DEPTH_U16 || a->format == RTXN_DEPTH_F32, "%s: unknown depth format %d (RTXN_DEPTH_U16 | _F32)", who, a->format);
  RTXN_REQUIRE(a->kind == RTXN_DEPTH_Z || a->kind == RTXN_DEPTH_RAY, "%s: unknown depth kind %d (RTXN_DEPTH_Z | _RAY)", who, a->kind);
  RTXN_REQUIRE(std::isfinite(a->scale) && a->scale > 0.0f, "%s: scale = %g (finite, > 0)", who, (double)a->scale);
  RTXN_REQUIRE(a->n_images >= 1, "%s: n_images = %d must be >= 1", who, a->n_images);
  RTXN_REQUIRE(a->n_rays >= 1, "%s: n_rays = %d must be >= 1", who, a->n_rays);
  RTXN_REQUIRE(a->width >= 1 && a->height >= 1 && (uint64_t)a->width * a->height <= (1ull << 24),
               "%s: %u x %u frames: width and height must be >= 1 and width*height <= 1 << 24", who, a->width, a->height);
  RTXN_DEVICE_OR_FAIL();
  const dim3 grid(((unsigned)a->n_rays + 255u) / 256u), block(256);
  hipStream_t st = rtxn::as_stream(stream);
  if (a->format == RTXN_DEPTH_U16) depth_targets_kernel<true><<<grid, block, 0, st>>>(*a);
  else depth_targets_kernel<false><<<grid, block, 0, st>>>(*a);
  RTXN_LAUNCH_CHECK("depth_targets_kernel");
  return RTXN_OK;
}
