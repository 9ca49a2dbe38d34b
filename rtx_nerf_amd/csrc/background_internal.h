// A training ray's background and the target it is fitted to (include/rtxn.h, rtxn_volrender_l2_train_ex), shared
// by the training compositors (volrender.hip, composite_train.hip) and the fixed-order loss sum (loss.hip) so that the loss is formed from the
// target the compositor fitted, bit for bit.  Internal to librtxn.so.  The struct stays in an anonymous namespace: the
// compositor's kernels take it by value and their symbols, pinned by tests/test_compositor_isa.py, carry its name.
#pragma once
#include "common.h"

namespace {

struct BgArgs {
  int mode;              // RTXN_BG_CONSTANT | RTXN_BG_RANDOM (loss.hip: also RTXN_BG_NONE, plain 3-channel targets)
  float color[3];        // CONSTANT
  unsigned seed;         // RANDOM
  const int* step;       // RANDOM: device int hashed with the seed, or NULL (0)
  int target_channels;   // 3 | 4 (straight RGBA, composited over the ray's background)
};

// the kernels' argument from the caller's struct; bg: an ACTIVE background, or NULL for plain 3-channel targets
inline BgArgs make_bg_args(const rtxn_train_background* bg) {
  BgArgs a{};
  a.mode = RTXN_BG_NONE;
  a.target_channels = 3;
  if (bg) {
    a.mode = bg->mode;
    for (int c = 0; c < 3; ++c) a.color[c] = bg->color[c];
    a.seed = bg->seed;
    a.step = bg->step;
    a.target_channels = bg->target_channels;
  }
  return a;
}

// the ray's background and its (composited) target: wave-uniform values
__device__ __forceinline__ void ray_background(const BgArgs& bg, const float* __restrict__ target, int ray, float (&b)[3],
                                               float (&t)[3]) {
  if (bg.mode == RTXN_BG_RANDOM) {
    const unsigned step = bg.step ? (unsigned)*bg.step : 0u;
    const unsigned h0 = rtxn::fmix32(bg.seed + 0x9E3779B9u * step);
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = (float)(rtxn::fmix32(h0 ^ (3u * (unsigned)ray + (unsigned)c)) >> 8) * 0x1p-24f;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = bg.color[c];
  }
  if (bg.target_channels == 4) {
    const float* p = target + 4 * (long)ray;
    const float a = p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = a * p[c] + (1.0f - a) * b[c];
  } else {
    const float* p = target + 3 * (long)ray;
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = p[c];
  }
}

}  // namespace
