// Held-out evaluation (rtxn_image_metrics, include/rtxn.h): mse, psnr and ssim of a rendered frame against one
// resident frame of an rtxn_image_set, as one record of three doubles in device memory.
//
// metrics_tile_kernel: a block owns a 16 x 16 tile of SSIM windows, i.e. a 26 x 26 halo of pixels of both images.  Every pixel
// of the frame belongs to exactly one block for the squared error (the tile its window origin would fall in; the last tile of
// a row / column also takes the 10 trailing pixels, which lie inside its halo), so the halo is read once for both metrics.
// With RTXN_METRICS_SSIM the halo is staged in LDS MINUS a per-tile pivot (each image's own pixel at the tile's centre, per channel), a
// horizontal pass leaves the five windowed sums (x, y, xx, yy, xy) per halo row and output column, a vertical pass finishes
// them per window -- fp32 fmaf chains in a fixed order -- and the moments and the quotient are formed in double.  The block
// reduces its squared error and its SSIM sum in double (DPP wave sum, then the four waves in order) to one partial each.
// metrics_fold_kernel: one block folds the partials in a fixed order and writes the record.  No atomics: the same bits every run.
//
// Bandwidth-trivial: an 800 x 800 frame is 7.7 MB of pred + 1.9 MB of RGB8 target, read once (halo overlap from L2).
#include <math.h>
#include "common.h"
#include "wave_scan_internal.h"

namespace {

constexpr int kTile = 16;                    // windows per tile side
constexpr int kWin = 11;                     // Gaussian window
constexpr int kHalo = kTile + kWin - 1;      // 26 pixels per tile side
constexpr int kThreads = kTile * kTile;      // one thread per window in the vertical pass
constexpr int kSums = 5;                     // x, y, xx, yy, xy

struct MetricsWindow {
  float w[kWin];       // exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, formed in double on the host and rounded to float
  double inv_weight;   // 1 / (sum of w)^2: what the rounding left of the 2-D window's weight, divided out of every windowed sum
};

// tiles along an axis of n pixels: ceil((n - 10) / 16) window tiles, one tile for a frame too small to hold a window
inline unsigned tiles_along(uint32_t n) { return n > (uint32_t)(kWin - 1) ? (n - (kWin - 1) + kTile - 1) / kTile : 1u; }

// the target pixel: batch.hip's read (F32 copied, U8 (float)v / 255.0f), a 4-channel one over the background
template <int C, bool U8>
__device__ __forceinline__ void read_target(const void* __restrict__ images, size_t pixel, const float (&bg)[3], float (&t)[3]) {
  float v[C];
  if (U8) {
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(images) + pixel * C;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (float)src[c] / 255.0f;
  } else {
    const float* __restrict__ src = static_cast<const float*>(images) + pixel * C;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = src[c];
  }
  if (C == 4) {
    const float a = v[C - 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = fmaf(a, v[c], (1.0f - a) * bg[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = v[c];
  }
}

template <int C, bool U8>
__global__ __launch_bounds__(kThreads) void metrics_tile_kernel(rtxn_image_metrics_args a, MetricsWindow win, unsigned tiles_x,
                                                                unsigned tiles_y) {
  __shared__ float img[2][3][kHalo][kHalo];           // pred, target: minus the pivot (16.2 KB)
  __shared__ float hs[kSums][3][kHalo][kTile];        // the horizontal pass (25.0 KB)
  __shared__ double red[kThreads / 64][2];
  const int tid = threadIdx.x;
  const unsigned W = a.set.width, H = a.set.height;
  const unsigned tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;     // blockIdx.x < tiles_x * tiles_y
  const unsigned x0 = tx * kTile, y0 = ty * kTile;                         // < W, < H
  const bool ssim = (a.flags & RTXN_METRICS_SSIM) != 0, clamp01 = (a.flags & RTXN_METRICS_CLAMP) != 0;
  const bool last_x = tx + 1 == tiles_x, last_y = ty + 1 == tiles_y;
  const size_t frame = (size_t)a.image * W * H;                            // first pixel of the frame in the set
  const float bg[3] = {a.background[0], a.background[1], a.background[2]};
  float pivot_p[3] = {0.0f, 0.0f, 0.0f}, pivot_t[3] = {0.0f, 0.0f, 0.0f};       // of pred and of the target: uniform over the block
  if (ssim) {
    // the centre of the part of the halo that lies inside the frame
    const unsigned cx = x0 + (min(x0 + kHalo, W) - x0) / 2, cy = y0 + (min(y0 + kHalo, H) - y0) / 2;      // < W, < H
    const size_t centre = (size_t)cy * W + cx;
    read_target<C, U8>(a.set.images, frame + centre, bg, pivot_t);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pivot_p[c] = a.pred[3 * centre + c];
      if (clamp01) pivot_p[c] = fminf(fmaxf(pivot_p[c], 0.0f), 1.0f);
    }
  }
  double se = 0.0;
  for (int i = tid; i < kHalo * kHalo; i += kThreads) {
    const int hx = i % kHalo, hy = i / kHalo;
    const unsigned gx = x0 + hx, gy = y0 + hy;
    float p[3] = {0.0f, 0.0f, 0.0f}, t[3] = {0.0f, 0.0f, 0.0f};
    const bool inside = gx < W && gy < H;
    if (inside) {
      const size_t pixel = (size_t)gy * W + gx;
      read_target<C, U8>(a.set.images, frame + pixel, bg, t);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[c] = a.pred[3 * pixel + c];
        if (clamp01) p[c] = fminf(fmaxf(p[c], 0.0f), 1.0f);
      }
      if ((hx < kTile || last_x) && (hy < kTile || last_y)) {              // this block's pixel for the squared error
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double d = (double)p[c] - (double)t[c];
          se += d * d;
        }
      }
    }
    if (ssim) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        img[0][c][hy][hx] = inside ? p[c] - pivot_p[c] : 0.0f;             // outside the frame: only windows that are not counted read it
        img[1][c][hy][hx] = inside ? t[c] - pivot_t[c] : 0.0f;
      }
    }
  }
  double ss = 0.0;
  if (ssim) {                                                              // uniform over the launch: every thread takes the barriers
    __syncthreads();
    for (int j = tid; j < 3 * kHalo * kTile; j += kThreads) {
      const int col = j % kTile, row = (j / kTile) % kHalo, c = j / (kTile * kHalo);
      float s[kSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const float x = img[0][c][row][col + k], y = img[1][c][row][col + k], wk = win.w[k];
        s[0] = fmaf(wk, x, s[0]);
        s[1] = fmaf(wk, y, s[1]);
        s[2] = fmaf(wk, x * x, s[2]);
        s[3] = fmaf(wk, y * y, s[3]);
        s[4] = fmaf(wk, x * y, s[4]);
      }
#pragma unroll
      for (int q = 0; q < kSums; ++q) hs[q][c][row][col] = s[q];
    }
    __syncthreads();
    const int ox = tid % kTile, oy = tid / kTile;
    if (x0 + ox < W - (kWin - 1) && y0 + oy < H - (kWin - 1)) {            // a valid window (W, H >= 11 under the flag)
      const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, inv_weight = win.inv_weight;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float s[kSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
          const float wk = win.w[k];
#pragma unroll
          for (int q = 0; q < kSums; ++q) s[q] = fmaf(wk, hs[q][c][oy + k][ox], s[q]);
        }
        const double mx = s[0] * inv_weight, my = s[1] * inv_weight;       // means minus the pivots
        const double vx = s[2] * inv_weight - mx * mx, vy = s[3] * inv_weight - my * my, cxy = s[4] * inv_weight - mx * my;
        const double ux = mx + (double)pivot_p[c], uy = my + (double)pivot_t[c];
        ss += ((2.0 * ux * uy + C1) * (2.0 * cxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
      }
    }
  }
  const double wse = wave_sum_d(se), wss = wave_sum_d(ss);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = wse;
    red[tid >> 6][1] = wss;
  }
  __syncthreads();
  if (tid == 0) {
    double r0 = red[0][0], r1 = red[0][1];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) {
      r0 += red[w][0];
      r1 += red[w][1];
    }
    double* partials = static_cast<double*>(a.workspace);
    partials[2 * (size_t)blockIdx.x] = r0;
    partials[2 * (size_t)blockIdx.x + 1] = r1;
  }
}

// one block: thread t folds partials t, t + 256, ... in ascending order, then the wave sum, then the four waves in order
__global__ __launch_bounds__(kThreads) void metrics_fold_kernel(const double* __restrict__ partials, unsigned n_tiles, double n_values,
                                                                double n_ssim, double* __restrict__ record) {
  __shared__ double red[kThreads / 64][2];
  const int tid = threadIdx.x;
  double se = 0.0, ss = 0.0;
  for (unsigned i = tid; i < n_tiles; i += kThreads) {
    se += partials[2 * (size_t)i];
    ss += partials[2 * (size_t)i + 1];
  }
  const double wse = wave_sum_d(se), wss = wave_sum_d(ss);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = wse;
    red[tid >> 6][1] = wss;
  }
  __syncthreads();
  if (tid == 0) {
    double r0 = red[0][0], r1 = red[0][1];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) {
      r0 += red[w][0];
      r1 += red[w][1];
    }
    const double mse = r0 / n_values;
    record[0] = mse;
    record[1] = mse <= 1e-12 ? 120.0 : 10.0 * log10(1.0 / mse);           // 10 log10(1 / max(mse, 1e-12))
    record[2] = n_ssim > 0.0 ? r1 / n_ssim : __builtin_nan("");
  }
}

// rtxn_draw_batch's rule for a frame size
bool frame_ok(uint32_t width, uint32_t height) { return width >= 1 && height >= 1 && (uint64_t)width * height <= (1ull << 24); }

}  // namespace

extern "C" size_t rtxn_image_metrics_workspace_bytes(uint32_t width, uint32_t height) {
  if (!frame_ok(width, height)) {
    rtxn::set_error("rtxn_image_metrics_workspace_bytes: %u x %u frames: width and height must be >= 1 and width*height <= 1 << 24",
                    width, height);
    return 0;
  }
  return (size_t)tiles_along(width) * tiles_along(height) * 2 * sizeof(double);
}

extern "C" int rtxn_image_metrics(const rtxn_image_metrics_args* a, rtxn_stream_t stream) {
  RTXN_REQUIRE(a != nullptr, "rtxn_image_metrics: args is NULL");
  const rtxn_image_set& s = a->set;
  RTXN_REQUIRE(s.images && a->pred, "rtxn_image_metrics: NULL images or pred");
  RTXN_REQUIRE(a->workspace && a->record, "rtxn_image_metrics: NULL workspace or record");
  RTXN_REQUIRE(((uintptr_t)a->workspace & 7) == 0 && ((uintptr_t)a->record & 7) == 0,
               "rtxn_image_metrics: workspace and record must be 8-byte aligned");
  RTXN_REQUIRE(s.n_images >= 1, "rtxn_image_metrics: n_images = %d must be >= 1", s.n_images);
  RTXN_REQUIRE(a->image >= 0 && a->image < s.n_images, "rtxn_image_metrics: image = %d outside [0, %d)", a->image, s.n_images);
  RTXN_REQUIRE(frame_ok(s.width, s.height),
               "rtxn_image_metrics: %u x %u frames: width and height must be >= 1 and width*height <= 1 << 24", s.width, s.height);
  RTXN_REQUIRE(s.channels == 3 || s.channels == 4, "rtxn_image_metrics: channels = %d must be 3 or 4", s.channels);
  RTXN_REQUIRE(s.format == RTXN_IMAGE_F32 || s.format == RTXN_IMAGE_U8, "rtxn_image_metrics: unknown image format %d", s.format);
  RTXN_REQUIRE((a->flags & ~(RTXN_METRICS_SSIM | RTXN_METRICS_CLAMP)) == 0, "rtxn_image_metrics: unknown flag bits in flags = %d",
               a->flags);
  const bool ssim = (a->flags & RTXN_METRICS_SSIM) != 0;
  RTXN_REQUIRE(!ssim || (s.width >= (uint32_t)kWin && s.height >= (uint32_t)kWin),
               "rtxn_image_metrics: RTXN_METRICS_SSIM needs frames of at least 11 x 11, not %u x %u", s.width, s.height);
  const unsigned tiles_x = tiles_along(s.width), tiles_y = tiles_along(s.height);
  const size_t need = (size_t)tiles_x * tiles_y * 2 * sizeof(double);
  RTXN_REQUIRE(a->workspace_bytes >= need, "rtxn_image_metrics: workspace_bytes = %zu, %u x %u frames need %zu", a->workspace_bytes,
               s.width, s.height, need);
  RTXN_DEVICE_OR_FAIL();
  MetricsWindow win;
  double g[kWin], sum = 0.0;
  for (int k = 0; k < kWin; ++k) {
    g[k] = exp(-(double)((k - kWin / 2) * (k - kWin / 2)) / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  double wsum = 0.0;
  for (int k = 0; k < kWin; ++k) {
    win.w[k] = (float)(g[k] / sum);
    wsum += (double)win.w[k];
  }
  win.inv_weight = 1.0 / (wsum * wsum);
  hipStream_t st = rtxn::as_stream(stream);
  const dim3 grid(tiles_x * tiles_y), block(kThreads);     // <= ceil(2^24 / 16) + 1 blocks
  const bool u8 = s.format == RTXN_IMAGE_U8;
  if (s.channels == 3) {
    if (u8) metrics_tile_kernel<3, true><<<grid, block, 0, st>>>(*a, win, tiles_x, tiles_y);
    else metrics_tile_kernel<3, false><<<grid, block, 0, st>>>(*a, win, tiles_x, tiles_y);
  } else {
    if (u8) metrics_tile_kernel<4, true><<<grid, block, 0, st>>>(*a, win, tiles_x, tiles_y);
    else metrics_tile_kernel<4, false><<<grid, block, 0, st>>>(*a, win, tiles_x, tiles_y);
  }
  RTXN_LAUNCH_CHECK("metrics_tile_kernel");
  const double n_values = 3.0 * (double)s.width * (double)s.height;
  const double n_ssim = ssim ? 3.0 * (double)(s.width - (kWin - 1)) * (double)(s.height - (kWin - 1)) : 0.0;
  metrics_fold_kernel<<<dim3(1), block, 0, st>>>(static_cast<const double*>(a->workspace), tiles_x * tiles_y, n_values, n_ssim,
                                                 a->record);
  RTXN_LAUNCH_CHECK("metrics_fold_kernel");
  return RTXN_OK;
}
