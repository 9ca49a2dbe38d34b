// The ray of a pixel under a camera model (rtxn_camera_set, include/rtxn.h states it operation for operation), shared by the ray
// generator (camera.hip) and the device batch draw (batch.hip) so that a ray drawn for training is the ray a frame of that camera
// walks, bit for bit -- the role make_ray (ray_internal.h) has for the centred pinhole.  Internal to librtxn.so.
#pragma once
#include "common.h"

namespace rtxn {

constexpr int kCameraNewtonSteps = 8;   // fp32 stops moving after 3 to 4 on every coefficient set of DESIGN 5.20; no early exit

// host only (camera.hip): the set's rules under `who`; n_images < 0: any n_cameras >= 1
int check_camera_set(const rtxn_camera_set* cameras, int n_images, const char* who);

// The OpenCV model's forward map at (x, y): the residual's two values before (xd, yd) is subtracted, and the symmetric Jacobian
// d(xd, yd) / d(x, y).  One body for the Newton solve below and for the intrinsics gradient (camera_refine.hip), which
// linearises at the solution.
__device__ __forceinline__ void opencv_forward(const float* __restrict__ cam, float x, float y, float& fx, float& fy, float& j11,
                                               float& j12, float& j22) {
  const float k1 = cam[4], k2 = cam[5], k3 = cam[6], p1 = cam[8], p2 = cam[9];
  const float xx = x * x, yy = y * y, xy = x * y;
  const float r2 = xx + yy;
  const float rad = fmaf(r2, fmaf(r2, fmaf(r2, k3, k2), k1), 1.0f);
  const float drad = fmaf(r2, fmaf(r2, 3.0f * k3, 2.0f * k2), k1);            // d rad / d r2
  fx = fmaf(x, rad, fmaf(2.0f * p1, xy, p2 * fmaf(2.0f, xx, r2)));
  fy = fmaf(y, rad, fmaf(2.0f * p2, xy, p1 * fmaf(2.0f, yy, r2)));
  j11 = fmaf(2.0f * xx, drad, rad) + fmaf(2.0f * p1, y, 6.0f * p2 * x);
  j22 = fmaf(2.0f * yy, drad, rad) + fmaf(2.0f * p2, x, 6.0f * p1 * y);
  j12 = fmaf(2.0f * xy, drad, 2.0f * fmaf(p1, x, p2 * y));                    // = j21
}

// (xd, yd) -> the undistorted (x, y) of the OpenCV radial-tangential model
__device__ __forceinline__ void undistort_opencv(const float* __restrict__ cam, float xd, float yd, float& x, float& y) {
  x = xd;
  y = yd;
#pragma unroll
  for (int it = 0; it < kCameraNewtonSteps; ++it) {
    float fx, fy, j11, j12, j22;
    opencv_forward(cam, x, y, fx, fy, j11, j12, j22);
    fx -= xd;
    fy -= yd;
    const float det = fmaf(j11, j22, -(j12 * j12));
    const bool ok = det != 0.0f && isfinite(det);
    const float dx = fmaf(j22, fx, -(j12 * fy)) / det;
    const float dy = fmaf(j11, fy, -(j12 * fx)) / det;
    x = ok ? x - dx : x;
    y = ok ? y - dy : y;
  }
}

// d (th poly(th)) / d th of the fisheye polynomial: the Newton solve's derivative, and the intrinsics gradient's
__device__ __forceinline__ float fisheye_dpoly(const float* __restrict__ cam, float th) {
  const float k1 = cam[4], k2 = cam[5], k3 = cam[6], k4 = cam[7];
  const float t2 = th * th;
  return fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, 9.0f * k4, 7.0f * k3), 5.0f * k2), 3.0f * k1), 1.0f);
}

// thd -> the undistorted angle of the OpenCV fisheye (equidistant polynomial) model
__device__ __forceinline__ float undistort_fisheye(const float* __restrict__ cam, float thd) {
  const float k1 = cam[4], k2 = cam[5], k3 = cam[6], k4 = cam[7];
  float th = thd;
#pragma unroll
  for (int it = 0; it < kCameraNewtonSteps; ++it) {
    const float t2 = th * th;
    const float poly = fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, k4, k3), k2), k1), 1.0f);
    const float dpoly = fisheye_dpoly(cam, th);
    const float f = fmaf(th, poly, -thd);
    const bool ok = dpoly != 0.0f && isfinite(dpoly);
    const float dth = f / dpoly;
    th = ok ? th - dth : th;
  }
  return th;
}

// cam: the camera's twelve floats; la: the row-major pose
template <int MODEL>
__device__ __forceinline__ void camera_ray(const float* __restrict__ cam, const float* __restrict__ la, unsigned px, unsigned py,
                                           float (&o)[3], float (&d)[3]) {
  const float xd = ((float)px + 0.5f - cam[2]) / cam[0];
  const float yd = ((float)py + 0.5f - cam[3]) / cam[1];
  float q0 = xd, q1 = yd, q2 = -1.0f;
  if (MODEL == RTXN_CAMERA_OPENCV) {
    undistort_opencv(cam, xd, yd, q0, q1);
  } else if (MODEL == RTXN_CAMERA_OPENCV_FISHEYE) {
    const float thd = sqrtf(fmaf(xd, xd, yd * yd));
    if (thd >= 1e-8f) {
      const float th = undistort_fisheye(cam, thd);
      const float s = sinf(th) / thd;
      q0 = s * xd;
      q1 = s * yd;
      q2 = -cosf(th);
    }
  }
  float x = fmaf(la[2], q2, fmaf(la[0], q0, la[1] * q1));
  float y = fmaf(la[6], q2, fmaf(la[4], q0, la[5] * q1));
  float z = fmaf(la[10], q2, fmaf(la[8], q0, la[9] * q1));
  const float norm = sqrtf(fmaf(z, z, fmaf(x, x, y * y)));
  d[0] = x / norm;
  d[1] = y / norm;
  d[2] = z / norm;
  o[0] = la[3] / 10;
  o[1] = la[7] / 10;
  o[2] = la[11] / 10;
}

}  // namespace rtxn
