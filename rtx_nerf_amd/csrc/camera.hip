// Camera models (rtxn_camera_set, include/rtxn.h): the ray generator that stands in front of the stages walking
// explicit rays.  One thread per launch pixel evaluates camera_ray (camera_internal.h) and stores the ray at its launch index:
// 64 B of pose and 48 B of camera shared by the whole launch, 24 B written per ray.
#include "common.h"
#include "camera_internal.h"

namespace {

template <int MODEL>
__global__ __launch_bounds__(256) void camera_rays_kernel(const float* __restrict__ cam, const float* __restrict__ la, unsigned width,
                                                          unsigned ray_begin, unsigned ray_count, float* __restrict__ rays_o,
                                                          float* __restrict__ rays_d) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= ray_count) return;   // tail block
  const unsigned gid = ray_begin + i;   // < width*height <= 2^31 - 1 (checked by the entry point)
  float o[3], d[3];
  rtxn::camera_ray<MODEL>(cam, la, gid % width, gid / width, o, d);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rays_o[3 * (size_t)gid + k] = o[k];
    rays_d[3 * (size_t)gid + k] = d[k];
  }
}

}  // namespace

int rtxn::check_camera_set(const rtxn_camera_set* c, int n_images, const char* who) {
  RTXN_REQUIRE(c != nullptr, "%s: cameras is NULL", who);
  RTXN_REQUIRE(c->model == RTXN_CAMERA_PINHOLE || c->model == RTXN_CAMERA_OPENCV || c->model == RTXN_CAMERA_OPENCV_FISHEYE,
               "%s: unknown camera model %d", who, c->model);
  if (n_images < 0)
    RTXN_REQUIRE(c->n_cameras >= 1, "%s: n_cameras = %d must be >= 1", who, c->n_cameras);
  else
    RTXN_REQUIRE(c->n_cameras == 1 || c->n_cameras == n_images, "%s: n_cameras = %d must be 1 or n_images = %d", who, c->n_cameras,
                 n_images);
  RTXN_REQUIRE(c->params != nullptr, "%s: NULL camera params", who);
  return RTXN_OK;
}

extern "C" int rtxn_camera_set_check(const rtxn_camera_set* cameras, int n_images) {
  RTXN_REQUIRE(n_images >= 1, "rtxn_camera_set_check: n_images = %d must be >= 1", n_images);
  return rtxn::check_camera_set(cameras, n_images, "rtxn_camera_set_check");
}

extern "C" int rtxn_camera_rays(const rtxn_camera_set* cameras, int camera, const float* look_at, uint32_t width, uint32_t height,
                                uint32_t ray_begin, uint32_t ray_count, float* rays_o, float* rays_d, rtxn_stream_t stream) {
  const char* who = "rtxn_camera_rays";
  int rc = rtxn::check_camera_set(cameras, -1, who);
  if (rc != RTXN_OK) return rc;
  RTXN_REQUIRE(camera >= 0 && camera < cameras->n_cameras, "%s: camera = %d out of [0,%d)", who, camera, cameras->n_cameras);
  RTXN_REQUIRE(look_at && rays_o && rays_d, "%s: NULL look_at, rays_o or rays_d", who);
  RTXN_REQUIRE(width >= 1 && height >= 1 && (uint64_t)width * height <= 0x7fffffffull,
               "%s: %u x %u frame: width and height must be >= 1 and width*height <= 2^31 - 1", who, width, height);
  RTXN_REQUIRE((uint64_t)ray_begin + ray_count <= (uint64_t)width * height, "%s: ray window [%u,+%u) exceeds the %ux%u frame", who,
               ray_begin, ray_count, width, height);
  RTXN_DEVICE_OR_FAIL();
  if (ray_count == 0) return RTXN_OK;
  const dim3 grid((ray_count + 255u) / 256u), block(256);
  hipStream_t st = rtxn::as_stream(stream);
  const float* cam = cameras->params + (size_t)RTXN_CAMERA_PARAMS * camera;
  switch (cameras->model) {
    case RTXN_CAMERA_PINHOLE:
      camera_rays_kernel<RTXN_CAMERA_PINHOLE><<<grid, block, 0, st>>>(cam, look_at, width, ray_begin, ray_count, rays_o, rays_d);
      break;
    case RTXN_CAMERA_OPENCV:
      camera_rays_kernel<RTXN_CAMERA_OPENCV><<<grid, block, 0, st>>>(cam, look_at, width, ray_begin, ray_count, rays_o, rays_d);
      break;
    default:
      camera_rays_kernel<RTXN_CAMERA_OPENCV_FISHEYE><<<grid, block, 0, st>>>(cam, look_at, width, ray_begin, ray_count, rays_o, rays_d);
      break;
  }
  RTXN_LAUNCH_CHECK("camera_rays_kernel");
  return RTXN_OK;
}
