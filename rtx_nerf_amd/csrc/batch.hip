// Training batches drawn on the device (rtxn_draw_batch, include/rtxn.h): replaces the reference's host batch build
// (std::random_shuffle + gather over a per-ray dataset, main.cu:612-629).  The frames stay resident as loaded, beside their
// poses; one thread per ray hashes (seed, step, ray) into an (image, pixel), generates that pixel's pinhole ray with the
// traversal's own make_ray (ray_internal.h) and copies the pixel's colour.  rtxn_draw_batch_cameras: the same draw with the ray
// from a camera model (camera_internal.h).
//
// A gather: per ray one 64-B pose (n_images of them in all, L2-resident), one 128-B line around the pixel (C or 4C bytes of it
// used) and 24 + 4C B written -- n_rays x (64 + 128 + 24 + 4C) B at worst, 0.9 MB for a 4096-ray RGB batch: launch latency, not
// bandwidth.
#include "common.h"
#include "ray_internal.h"
#include "camera_internal.h"

namespace {

// h0 is uniform over the launch: one scalar load, hashed once per wave.
__device__ __forceinline__ unsigned draw_h0(unsigned seed, const int* step) {
  const unsigned t = step ? (unsigned)*step : 0u;
  return rtxn::fmix32((seed ^ 0x2C1B3C6Du) + 0x9E3779B9u * t);
}

// multiply-shift: h uniform over 2^32 -> [0, n)
__device__ __forceinline__ unsigned draw_index(unsigned h, unsigned n) {
  return (unsigned)(((unsigned long long)h * (unsigned long long)n) >> 32);
}

template <int C, bool U8>
__global__ __launch_bounds__(256) void draw_batch_kernel(rtxn_draw_batch_args a) {
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  if (r >= (unsigned)a.n_rays) return;   // tail block
  const unsigned h0 = draw_h0(a.seed, a.step);
  const unsigned n_pixels = a.set.width * a.set.height;   // <= 1 << 24 (checked by the entry point)
  const unsigned image = draw_index(rtxn::fmix32(h0 ^ (2u * r)), (unsigned)a.set.n_images);
  const unsigned pixel = draw_index(rtxn::fmix32(h0 ^ (2u * r + 1u)), n_pixels);
  float o[3], d[3], v[2];
  rtxn::make_ray(a.set.poses + 16 * (size_t)image, a.set.focal_length, a.set.aspect_ratio, a.set.width, a.set.height,
                 pixel % a.set.width, pixel / a.set.width, o, d, v);
  const size_t texel = ((size_t)image * n_pixels + pixel) * C;
  float t[C];
  if (U8) {
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(a.set.images) + texel;
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = (float)src[c] / 255.0f;
  } else {
    const float* __restrict__ src = static_cast<const float*>(a.set.images) + texel;
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = src[c];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.rays_o[3 * (size_t)r + k] = o[k];
    a.rays_d[3 * (size_t)r + k] = d[k];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) a.targets[C * (size_t)r + c] = t[c];
  if (a.drawn) {
    a.drawn[2 * (size_t)r] = image;
    a.drawn[2 * (size_t)r + 1] = pixel;
  }
}

// The same draw with the pixel's ray from a camera model (camera_internal.h): the hash sequence, the texel and the stores are
// draw_batch_kernel's, so (image, pixel) and the target bits are too; the set's focal_length / aspect_ratio are not read.
template <int C, bool U8, int MODEL>
__global__ __launch_bounds__(256) void draw_batch_cameras_kernel(rtxn_draw_batch_args a, rtxn_camera_set cams) {
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  if (r >= (unsigned)a.n_rays) return;   // tail block
  const unsigned h0 = draw_h0(a.seed, a.step);
  const unsigned n_pixels = a.set.width * a.set.height;
  const unsigned image = draw_index(rtxn::fmix32(h0 ^ (2u * r)), (unsigned)a.set.n_images);
  const unsigned pixel = draw_index(rtxn::fmix32(h0 ^ (2u * r + 1u)), n_pixels);
  const float* cam = cams.params + (size_t)RTXN_CAMERA_PARAMS * (cams.n_cameras == 1 ? 0u : image);
  float o[3], d[3];
  rtxn::camera_ray<MODEL>(cam, a.set.poses + 16 * (size_t)image, pixel % a.set.width, pixel / a.set.width, o, d);
  const size_t texel = ((size_t)image * n_pixels + pixel) * C;
  float t[C];
  if (U8) {
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(a.set.images) + texel;
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = (float)src[c] / 255.0f;
  } else {
    const float* __restrict__ src = static_cast<const float*>(a.set.images) + texel;
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = src[c];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.rays_o[3 * (size_t)r + k] = o[k];
    a.rays_d[3 * (size_t)r + k] = d[k];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) a.targets[C * (size_t)r + c] = t[c];
  if (a.drawn) {
    a.drawn[2 * (size_t)r] = image;
    a.drawn[2 * (size_t)r + 1] = pixel;
  }
}

// rtxn_draw_batch's argument rules (include/rtxn.h), host only, under the entry point's name
int check_draw_batch(const rtxn_draw_batch_args* a, const char* who) {
  RTXN_REQUIRE(a != nullptr, "%s: args is NULL", who);
  const rtxn_image_set& s = a->set;
  RTXN_REQUIRE(s.images && s.poses, "%s: NULL images or poses", who);
  RTXN_REQUIRE(a->rays_o && a->rays_d && a->targets, "%s: NULL rays_o, rays_d or targets", who);
  RTXN_REQUIRE(s.n_images >= 1, "%s: n_images = %d must be >= 1", who, s.n_images);
  RTXN_REQUIRE(a->n_rays >= 1, "%s: n_rays = %d must be >= 1", who, a->n_rays);
  RTXN_REQUIRE(s.width >= 1 && s.height >= 1 && (uint64_t)s.width * s.height <= (1ull << 24),
               "%s: %u x %u frames: width and height must be >= 1 and width*height <= 1 << 24", who, s.width, s.height);
  RTXN_REQUIRE(s.channels == 3 || s.channels == 4, "%s: channels = %d must be 3 or 4", who, s.channels);
  RTXN_REQUIRE(s.format == RTXN_IMAGE_F32 || s.format == RTXN_IMAGE_U8, "%s: unknown image format %d", who, s.format);
  return RTXN_OK;
}

template <int MODEL>
void launch_cameras(const rtxn_draw_batch_args& a, const rtxn_camera_set& cams, dim3 grid, hipStream_t st) {
  const dim3 block(256);
  const bool u8 = a.set.format == RTXN_IMAGE_U8;
  if (a.set.channels == 3) {
    if (u8) draw_batch_cameras_kernel<3, true, MODEL><<<grid, block, 0, st>>>(a, cams);
    else draw_batch_cameras_kernel<3, false, MODEL><<<grid, block, 0, st>>>(a, cams);
  } else {
    if (u8) draw_batch_cameras_kernel<4, true, MODEL><<<grid, block, 0, st>>>(a, cams);
    else draw_batch_cameras_kernel<4, false, MODEL><<<grid, block, 0, st>>>(a, cams);
  }
}

}  // namespace

extern "C" int rtxn_draw_batch(const rtxn_draw_batch_args* a, rtxn_stream_t stream) {
  int rc = check_draw_batch(a, "rtxn_draw_batch");
  if (rc != RTXN_OK) return rc;
  const rtxn_image_set& s = a->set;
  RTXN_DEVICE_OR_FAIL();
  const dim3 grid(((unsigned)a->n_rays + 255u) / 256u), block(256);
  hipStream_t st = rtxn::as_stream(stream);
  const bool u8 = s.format == RTXN_IMAGE_U8;
  if (s.channels == 3) {
    if (u8) draw_batch_kernel<3, true><<<grid, block, 0, st>>>(*a);
    else draw_batch_kernel<3, false><<<grid, block, 0, st>>>(*a);
  } else {
    if (u8) draw_batch_kernel<4, true><<<grid, block, 0, st>>>(*a);
    else draw_batch_kernel<4, false><<<grid, block, 0, st>>>(*a);
  }
  RTXN_LAUNCH_CHECK("draw_batch_kernel");
  return RTXN_OK;
}

extern "C" int rtxn_draw_batch_cameras(const rtxn_draw_batch_args* a, const rtxn_camera_set* cameras, rtxn_stream_t stream) {
  const char* who = "rtxn_draw_batch_cameras";
  int rc = check_draw_batch(a, who);
  if (rc != RTXN_OK) return rc;
  rc = rtxn::check_camera_set(cameras, a->set.n_images, who);
  if (rc != RTXN_OK) return rc;
  RTXN_DEVICE_OR_FAIL();
  const dim3 grid(((unsigned)a->n_rays + 255u) / 256u);
  hipStream_t st = rtxn::as_stream(stream);
  switch (cameras->model) {
    case RTXN_CAMERA_PINHOLE: launch_cameras<RTXN_CAMERA_PINHOLE>(*a, *cameras, grid, st); break;
    case RTXN_CAMERA_OPENCV: launch_cameras<RTXN_CAMERA_OPENCV>(*a, *cameras, grid, st); break;
    default: launch_cameras<RTXN_CAMERA_OPENCV_FISHEYE>(*a, *cameras, grid, st); break;
  }
  RTXN_LAUNCH_CHECK("draw_batch_cameras_kernel");
  return RTXN_OK;
}
