// The pinhole ray of a launch pixel, shared by the traversal (trace.hip) and the device batch draw (batch.hip) so that a ray
// drawn for training is the ray the traversal would generate for that pixel, bit for bit.  Internal to librtxn.so.
#pragma once
#include "common.h"

namespace rtxn {

// a2: optixPrograms.cu:43-82
__device__ __forceinline__ void make_ray(const float* __restrict__ la, float focal_length, float aspect_ratio,
                                         unsigned width, unsigned height, unsigned px, unsigned py, float (&o)[3],
                                         float (&d)[3], float (&v)[2]) {
  const float u = (float)((2 * (px + 0.5) / width - 1) * aspect_ratio);
  const float vv = (float)(2 * (py + 0.5) / height - 1);
  const float nf0 = la[2] * -1.0f, nf1 = la[6] * -1.0f, nf2 = la[10] * -1.0f;
  float xd = fmaf(nf0, focal_length, fmaf(la[0], u, la[1] * vv));
  float yd = fmaf(nf1, focal_length, fmaf(la[4], u, la[5] * vv));
  float zd = fmaf(nf2, focal_length, fmaf(la[8], u, la[9] * vv));
  const float norm = sqrtf(fmaf(zd, zd, fmaf(xd, xd, yd * yd)));
  xd /= norm;
  yd /= norm;
  zd /= norm;
  v[0] = atan2f(sqrtf(fmaf(xd, xd, yd * yd)), zd);
  v[1] = atan2f(yd, xd);
  d[0] = xd; d[1] = yd; d[2] = zd;
  o[0] = la[3] / 10;
  o[1] = la[7] / 10;
  o[2] = la[11] / 10;
}

}  // namespace rtxn
