// Occupancy refresh on the device (rtxn_occupancy_refresh, include/rtxn.h): evaluate sigma at one point per cell of the R^3
// grid with the fused INFERENCE kernels, fold it into a decaying running maximum, threshold, rebuild the traversal hierarchy
// in place.  No counterpart in the reference, which builds the dense grid once (main.cu:393-399); the rule is instant-ngp's
// (Mueller et al. 2022, section "Accelerated ray marching": density grid = max(decayed grid, new sample), threshold
// min(given, mean)).  Nothing here synchronises, reads back or allocates: the entry is hipGraph-capturable.
//
// A RUN AS A SEGMENT.  The inference kernels shade packed segments: 32 REGULAR samples at start + (i/32)(end - start).  Cells
// (x, y, 32k .. 32k+31) of the grid lie on a line, one cell apart: with start = the first cell's sample point and end = start +
// 32 cells along z, sample i of that pseudo-segment IS the sample point of cell z = 32k + i.  There are NK = ceil(R/32) runs
// per row (x, y) and R*R*NK runs in all, global run index g = (x*R + y)*NK + k; samples of a tail run with 32k + i >= R are
// shaded and dropped.  seg_view = (0, 0).  A pass generates `runs_per_pass` runs into the workspace, shades them
// (rtxn_hashmlp_forward_segments, REGULAR, or rtxn_mlp_forward_segments_compact: both write half[.][4], sigma = component 3,
// the value the compositor consumes) and folds them; ceil(runs / runs_per_pass) passes, a host-side trip count.
//
// THE ARITHMETIC, float32 throughout, every operation rounded on its own (no contraction into fma), in this order:
//   h      = 2.0f / (float)R
//   p_x    = ((float)x + 0.5f) * h - 1.0f          p_y likewise from y, p_z from z0 = 32k
//   jitter = 0:  start = (p_x, p_y, p_z)
//   jitter != 0: step = (uint32)*step (NULL: 0);  h0 = fmix32(seed + 0x9E3779B9u * step)   (uint32 wrap-around; fmix32 =
//                MurmurHash3's finaliser, the hash of RTXN_BG_RANDOM);  for c = 0, 1, 2 (x, y, z):
//                u_c = (float)(fmix32(h0 ^ (3u * g + c)) >> 8) * 2^-24   (24 hash bits, exact, in [0, 1))
//                start_c = p_c + (u_c - 0.5f) * h
//                ONE offset per run, shared by its 32 cells: a segment's samples are equally spaced on a line, so the only
//                jitter it can carry is a translation of the whole run.
//   end    = (start_x, start_y, start_z + 32.0f * h)
// Fold, for every cell c = (x*R + y)*R + z of the run with z = 32k + i < R, s = (float) of the half sigma of sample i:
//   s != s (NaN): s = 0;   v = s * thickness_scale;   d = density[c] * decay;   density[c] = v > d ? v : d
// Sum of the new density: per run, the 32 lane values t_i (0 for z >= R) are added as a butterfly --
//   for o in 16, 8, 4, 2, 1: t_i = t_i + t_(i xor o)   -- into partial[g] (float); the partials are then summed in double, lane
// j of a 1024-thread block taking g = j, j + 1024, ... in ascending order, followed by a binary tree over the lanes.  Both orders
// are fixed by g alone, so the sum does not depend on how the runs are cut into passes or on which wave finishes first.
//   mean = (float)(sum / (double)R^3);   thr = threshold (RTXN_OCC_ABSOLUTE) | fminf(threshold, mean) (RTXN_OCC_MIN_MEAN)
//   bit c = density[c] > thr;  tail bits of the last word 0;  *occupied = number of set bits (integer atomics).
// The 4^3 mip, the bricks and the 16^3 mip come from the existing builders (trace.hip), fed the new bits.
//
// HBM per cell: the fold reads 8 B of radiance and 4 B of density and writes 4 B; the threshold pass reads 4 B and writes a
// bit.  Both kernels are one lane per cell, consecutive lanes consecutive z: every array is touched with one coalesced access
// per wave, sums and bits are formed with wave shuffles / ballot.  The shading kernels dominate.
#include "common.h"

#include "mlp_internal.h"

namespace {

using rtxn::fmix32;

constexpr int kK = RTXN_NUM_SAMPLES_PER_SEGMENT;   // 32 cells per run
constexpr long kMaxRunsPerPass = 1L << 25;         // = the runs of the largest grid (R = 1024)

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// [start float3[P] | end float3[P] | seg_view float2[P] | radiance half4[32 P] | partial float[runs] | count, mean, thr]
struct Layout {
  size_t start, end, view, radiance, partials, scalars, total;
};

Layout layout_of(int R, long P) {
  const long nk = (R + kK - 1) / kK, runs = (long)R * R * nk;
  Layout l;
  size_t o = 0;
  l.start = o;    o += up256((size_t)P * 12);
  l.end = o;      o += up256((size_t)P * 12);
  l.view = o;     o += up256((size_t)P * 8);
  l.radiance = o; o += up256((size_t)P * kK * 8);
  l.partials = o; o += up256((size_t)runs * 4);
  l.scalars = o;  o += 256;
  l.total = o;
  return l;
}

struct Scalars {
  int count;     // segments of the current pass
  float mean;
  float thr;
};

struct GenArgs {
  int R, nk;
  long base, n_pass;     // first global run of the pass, runs in it
  int jitter;
  unsigned seed;
  const int* step;
  float* start;
  float* end;
  float* view;
  int* count;
};

// one thread per run of the pass: the pseudo-segment records and the pass's segment count
__global__ __launch_bounds__(256) void occ_generate_kernel(GenArgs a) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) *a.count = (int)a.n_pass;
  if (t >= a.n_pass) return;
  const long g = a.base + t;
  const int k = (int)(g % a.nk);
  const long row = g / a.nk;
  const int y = (int)(row % a.R), x = (int)(row / a.R);
  const float h = 2.0f / (float)a.R;
  float p[3] = {((float)x + 0.5f) * h - 1.0f, ((float)y + 0.5f) * h - 1.0f, ((float)(kK * k) + 0.5f) * h - 1.0f};
  if (a.jitter) {
    const unsigned step = a.step ? (unsigned)*a.step : 0u;
    const unsigned h0 = fmix32(a.seed + 0x9E3779B9u * step);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float u = (float)(fmix32(h0 ^ (3u * (unsigned)g + (unsigned)c)) >> 8) * 0x1p-24f;
      p[c] = p[c] + (u - 0.5f) * h;
    }
  }
  a.start[3 * t + 0] = p[0];
  a.start[3 * t + 1] = p[1];
  a.start[3 * t + 2] = p[2];
  a.end[3 * t + 0] = p[0];
  a.end[3 * t + 1] = p[1];
  a.end[3 * t + 2] = p[2] + 32.0f * h;
  a.view[2 * t + 0] = 0.0f;
  a.view[2 * t + 1] = 0.0f;
}

struct FoldArgs {
  int R, nk;
  long base, n_pass;
  const uint2* radiance;   // half4 per sample
  float* density;
  float decay, thickness_scale;
  float* partials;
};

// one lane per sample of the pass (a wave = two runs): density = max(density * decay, sigma * thickness_scale), and the run's sum
__global__ __launch_bounds__(256) void occ_fold_kernel(FoldArgs a) {
#pragma clang fp contract(off)
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const long t = s >> 5;
  const int i = (int)(s & 31);
  const bool run_ok = t < a.n_pass;
  const long g = a.base + (run_ok ? t : 0);
  const int k = (int)(g % a.nk);
  const long row = g / a.nk;
  const int z = kK * k + i;
  float val = 0.0f;
  if (run_ok && z < a.R) {
    const uint2 q = a.radiance[s];
    float sigma = (float)__ushort_as_half((unsigned short)(q.y >> 16));
    if (!(sigma == sigma)) sigma = 0.0f;
    const float v = sigma * a.thickness_scale;
    const long c = row * a.R + z;
    const float d = a.density[c] * a.decay;
    val = v > d ? v : d;
    a.density[c] = val;
  }
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) val = val + __shfl_xor(val, o, 64);
  if (run_ok && i == 0) a.partials[g] = val;
}

struct ReduceArgs {
  const float* partials;
  long runs;
  double n_cells;
  float threshold;
  int min_mean;
  Scalars* sc;
  float* mean_out;
  int* occupied;
};

// one block: the partials in a fixed order -> mean and threshold; clears the popcount the bit kernel adds to
__global__ __launch_bounds__(1024) void occ_reduce_kernel(ReduceArgs a) {
  __shared__ double part[1024];
  const int j = threadIdx.x;
  double acc = 0.0;
  for (long g = j; g < a.runs; g += 1024) acc += (double)a.partials[g];
  part[j] = acc;
  __syncthreads();
  for (int w = 512; w >= 1; w >>= 1) {
    if (j < w) part[j] += part[j + w];
    __syncthreads();
  }
  if (j == 0) {
    const float mean = (float)(part[0] / a.n_cells);
    a.sc->mean = mean;
    a.sc->thr = a.min_mean ? fminf(a.threshold, mean) : a.threshold;
    if (a.mean_out) *a.mean_out = mean;
    if (a.occupied) *a.occupied = 0;
  }
}

// occupancy_kernel (trace.hip) with the threshold on the device and a popcount: one ballot = two words; a block walks its
// chunks with a grid stride and adds its count once
__global__ __launch_bounds__(256) void occ_bits_kernel(const float* __restrict__ density, const Scalars* __restrict__ sc, long n,
                                                       long padded_n, uint32_t* __restrict__ bits, int* __restrict__ occupied) {
  __shared__ int block_count;
  if (threadIdx.x == 0) block_count = 0;
  __syncthreads();
  const float thr = sc->thr;
  const int lane = threadIdx.x & 63;
  int count = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < padded_n; i += (long)gridDim.x * 256) {   // padded_n: a multiple of 64
    const bool on = i < n && density[i] > thr;
    const unsigned long long m = __ballot(on);
    if ((lane & 31) == 0 && (i & ~31L) < n) bits[i >> 5] = (uint32_t)(m >> (lane & 32));
    count += __popcll(m);           // wave-uniform
  }
  if (occupied) {
    if (lane == 0 && count) atomicAdd(&block_count, count);
    __syncthreads();
    if (threadIdx.x == 0 && block_count) atomicAdd(occupied, block_count);
  }
}

bool supported(const rtxn_mlp* m, const rtxn_hashgrid* g, int n_dir_freqs) {
  if (!m) return false;
  if (g) return rtxn_hashmlp_supported(m, g, n_dir_freqs) != 0;
  return m->variant >= 0;       // what rtxn_mlp_forward_segments_compact accepts: a model with a fused inference kernel
}

}  // namespace

extern "C" int rtxn_occupancy_refresh_supported(const rtxn_mlp* m, const rtxn_hashgrid* g, int n_dir_freqs) {
  return supported(m, g, n_dir_freqs) ? 1 : 0;
}

extern "C" size_t rtxn_occupancy_refresh_workspace_bytes(int grid_res, long runs_per_pass) {
  if (grid_res < 1 || grid_res > 1024) {
    rtxn::set_error("rtxn_occupancy_refresh_workspace_bytes: grid_res = %d out of [1,1024]", grid_res);
    return 0;
  }
  if (runs_per_pass < 1 || runs_per_pass > kMaxRunsPerPass) {
    rtxn::set_error("rtxn_occupancy_refresh_workspace_bytes: runs_per_pass = %ld out of [1,%ld]", runs_per_pass, kMaxRunsPerPass);
    return 0;
  }
  return layout_of(grid_res, runs_per_pass).total;
}

extern "C" int rtxn_occupancy_refresh(const rtxn_occupancy_refresh_args* a, rtxn_stream_t stream) {
  RTXN_REQUIRE(a != nullptr, "rtxn_occupancy_refresh: NULL args");
  RTXN_REQUIRE(a->mlp != nullptr, "rtxn_occupancy_refresh: NULL model");
  const int R = a->grid_res;
  RTXN_REQUIRE(R >= 1 && R <= 1024, "rtxn_occupancy_refresh: grid_res = %d out of [1,1024]", R);
  RTXN_REQUIRE(a->density != nullptr, "rtxn_occupancy_refresh: NULL density");
  RTXN_REQUIRE(a->decay >= 0.0f && a->decay <= 1.0f, "rtxn_occupancy_refresh: decay = %g outside [0,1]", (double)a->decay);
  RTXN_REQUIRE(a->threshold_mode == RTXN_OCC_ABSOLUTE || a->threshold_mode == RTXN_OCC_MIN_MEAN,
               "rtxn_occupancy_refresh: unknown threshold mode %d", a->threshold_mode);
  RTXN_REQUIRE(a->occupancy != nullptr, "rtxn_occupancy_refresh: NULL occupancy");
  // the hierarchy levels exist exactly where the traversal can use them
  RTXN_REQUIRE((a->coarse != nullptr) == (R % 4 == 0), "rtxn_occupancy_refresh: coarse must be %s for grid_res = %d (grid_res %% 4 %s 0)",
               R % 4 == 0 ? "given" : "NULL", R, R % 4 == 0 ? "==" : "!=");
  RTXN_REQUIRE((a->bricks != nullptr) == (R % 4 == 0), "rtxn_occupancy_refresh: bricks must be %s for grid_res = %d (grid_res %% 4 %s 0)",
               R % 4 == 0 ? "given" : "NULL", R, R % 4 == 0 ? "==" : "!=");
  RTXN_REQUIRE((a->super_mip != nullptr) == (R % 16 == 0),
               "rtxn_occupancy_refresh: super_mip must be %s for grid_res = %d (grid_res %% 16 %s 0)", R % 16 == 0 ? "given" : "NULL", R,
               R % 16 == 0 ? "==" : "!=");
  RTXN_REQUIRE(!a->grid || a->table_fp16, "rtxn_occupancy_refresh: a hash grid needs its table (table_fp16 is NULL)");
  if (!supported(a->mlp, a->grid, a->n_dir_freqs)) {
    rtxn::set_error("rtxn_occupancy_refresh: no fused inference kernel for this model (%s); evaluate the cells through the training "
                    "entry points instead",
                    a->grid ? "hash grid: rtxn_hashmlp_supported is 0" : "pre-encoded model without a grid");
    return RTXN_ERR_UNSUPPORTED;
  }
  const long P = a->runs_per_pass;
  RTXN_REQUIRE(P >= 1 && P <= kMaxRunsPerPass, "rtxn_occupancy_refresh: runs_per_pass = %ld out of [1,%ld]", P, kMaxRunsPerPass);
  const Layout lay = layout_of(R, P);
  RTXN_REQUIRE(a->workspace != nullptr && ((uintptr_t)a->workspace & 255) == 0,
               "rtxn_occupancy_refresh: the workspace must be given and 256-byte aligned");
  RTXN_REQUIRE(a->workspace_bytes >= lay.total,
               "rtxn_occupancy_refresh: workspace of %zu bytes is too small, rtxn_occupancy_refresh_workspace_bytes(%d, %ld) = %zu",
               a->workspace_bytes, R, P, lay.total);
  RTXN_DEVICE_OR_FAIL();
  RTXN_REQUIRE(a->mlp->packed && a->mlp->inference_ready,
               "rtxn_occupancy_refresh: the fused inference kernels' weights are not current: call rtxn_mlp_set_params first");

  hipStream_t s = rtxn::as_stream(stream);
  uint8_t* ws = static_cast<uint8_t*>(a->workspace);
  float* start = reinterpret_cast<float*>(ws + lay.start);
  float* end = reinterpret_cast<float*>(ws + lay.end);
  float* view = reinterpret_cast<float*>(ws + lay.view);
  void* radiance = ws + lay.radiance;
  float* partials = reinterpret_cast<float*>(ws + lay.partials);
  Scalars* sc = reinterpret_cast<Scalars*>(ws + lay.scalars);
  const int nk = (R + kK - 1) / kK;
  const long runs = (long)R * R * nk;

  for (long base = 0; base < runs; base += P) {
    const long n_pass = runs - base < P ? runs - base : P;
    GenArgs ga{R, nk, base, n_pass, a->jitter, a->seed, a->step, start, end, view, &sc->count};
    occ_generate_kernel<<<(unsigned)((n_pass + 255) / 256), 256, 0, s>>>(ga);
    RTXN_LAUNCH_CHECK("occ_generate_kernel");
    int rc;
    if (a->grid)
      rc = rtxn_hashmlp_forward_segments(a->mlp, a->grid, a->n_dir_freqs, a->table_fp16, start, end, view, &sc->count, n_pass,
                                         RTXN_SAMPLING_REGULAR, 1.0f, radiance, nullptr, stream);
    else
      rc = rtxn_mlp_forward_segments_compact(a->mlp, start, end, view, &sc->count, n_pass, radiance, stream);
    if (rc != RTXN_OK) return rc;
    FoldArgs fa{R, nk, base, n_pass, static_cast<const uint2*>(radiance), a->density, a->decay, a->thickness_scale, partials};
    occ_fold_kernel<<<(unsigned)((n_pass * kK + 255) / 256), 256, 0, s>>>(fa);
    RTXN_LAUNCH_CHECK("occ_fold_kernel");
  }

  const long n = (long)R * R * R;
  ReduceArgs ra{partials, runs, (double)n, a->threshold, a->threshold_mode == RTXN_OCC_MIN_MEAN, sc, a->mean, a->occupied};
  occ_reduce_kernel<<<1, 1024, 0, s>>>(ra);
  RTXN_LAUNCH_CHECK("occ_reduce_kernel");
  const long padded_n = (n + 63) / 64 * 64;
  const long blocks = (padded_n + 255) / 256;
  occ_bits_kernel<<<(unsigned)(blocks > 1024 ? 1024 : blocks), 256, 0, s>>>(a->density, sc, n, padded_n, a->occupancy, a->occupied);
  RTXN_LAUNCH_CHECK("occ_bits_kernel");
  int rc = RTXN_OK;
  if (a->coarse) rc = rtxn_build_occupancy_mip(a->occupancy, R, a->coarse, stream);
  if (rc == RTXN_OK && a->bricks) rc = rtxn_build_occupancy_bricks(a->occupancy, R, a->bricks, stream);
  if (rc == RTXN_OK && a->super_mip) rc = rtxn_build_occupancy_mip(a->coarse, R / 4, a->super_mip, stream);
  return rc;
}
