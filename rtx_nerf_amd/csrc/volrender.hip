// Alpha-compositing volume renderer, forward and backward.
// Replaces volrender_cuda / volrender_backward_cuda and their launchers
// (reference vol_render/vol_render.cu:19-190).
//
// The reference walks a ray's samples serially in one thread.  Here one
// 64-lane wavefront owns a ray and consumes 64 consecutive samples per step
// (a ray's samples are contiguous: [indices[r]*K, (indices[r]+num_hits[r])*K)):
// coalesced 16-B radiance loads (1 KiB per wave instruction), the optical depth
// running sum as a wavefront-wide inclusive prefix scan carried across steps,
// and a final cross-lane reduction of the weighted colour.
//
// HBM-bound.  Algorithmic bytes: forward 20 B/sample (16 radiance + 4 t) + 20
// B/ray; backward 20 B/sample read + 8 B/sample written + 14 B/ray.
//
// RTXN_VR_COMPAT reproduces the reference arithmetic:
//   delta_i = |t_i - t_{i-1}|, t_{-1} = 0, NOT reset at segment boundaries;
//   T_i = sum_{k<=i} delta_k sigma_k (inclusive); w_i = exp(-T_i)(1-exp(-delta_i sigma_i)).
// The scan sums in a different order than the reference's serial loop, hence
// the 1e-5 absolute tolerance on pixels stated in tests/.
// RTXN_VR_NERF is the canonical quadrature (exclusive transmittance, ray_hit
// holds each sample's world-space step length) with its exact gradient.
#include <type_traits>

#include "background_internal.h"
#include "common.h"
#include "wave_scan_internal.h"

namespace {

// Colour, opacity A = sum w_i and expected depth sum w_i d_i in one pass (rtxn_volrender_fwd_aux): the forward kernels with two
// more accumulators.  One-sample schedule: ONE body, fwd_body<MODE, COMPACT, AUX>, instantiated by volrender_fwd_kernel
// (AUX = false) and volrender_aux_kernel (AUX = true); everything the extended form adds sits under `if constexpr (AUX)`, so
// with a zero background the pixels are bit-identical by construction.  Pair schedule: volrender_aux_pair_kernel is still a
// copy of volrender_fwd_pair_kernel with the additions written in, weights and colour accumulation operation for operation
// (a body that is inlined into a kernel is optimised once on its own and once more inside the kernel, and for the pair and
// the training kernels that second round changes the code of the plain kernel, whose measurements are keyed on its bytes:
// DESIGN 5.5).  tests/test_compositor_isa.py pins the machine code of every kernel here.
// d_i = t_start_j + u_i (t_end_j - t_start_j) is the distance at which sample i of segment j
// was evaluated: u_i = (i + u0) / K (u0 = 0 REGULAR, 0.5 MIDPOINT_WORLD); t_start / t_end (one float each per segment, 8 B per
// K samples) are read only when depth is requested.  The background is added per channel where it is non-zero:
// pixel += (1 - A) bg (no 0 * x term, which would turn a -0.0 pixel into +0.0).
struct AuxArgs {
  const float* t_start;
  const float* t_end;
  float u0;
  float bg[3];
  float* depth;     // may be NULL
  float* opacity;   // may be NULL
};

// COMPACT: radiance is half[N][4] (the network's own output, 8 B/sample instead of 16) and per-sample t_vals are not read at
// all.  RTXN_VR_COMPAT: REGULAR sampling makes them the function (i + 1) / K of the sample index (sampler.cu:52-66);
// RTXN_VR_NERF: every sample of a segment has the same world-space step, so `ray_hit` is one float per SEGMENT (4 B per K
// samples).  Same arithmetic from there on, so the pixels are bit-identical to the float4 + t_vals form at 40 % of its bytes.
template <int MODE, bool COMPACT, bool AUX>
__device__ __forceinline__ void fwd_body(const float4* __restrict__ radiance, const int* __restrict__ num_hits,
                                         const int* __restrict__ indices, const float* __restrict__ ray_hit, int batch_size, int K,
                                         float* __restrict__ pixels, const AuxArgs& aux) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= batch_size) return;
  const long seg = indices[ray];
  const long base = seg * K;
  const long n = (long)num_hits[ray] * K;
  const bool want_depth = AUX && aux.depth != nullptr;
  float T_carry = 0.0f, t_carry = 0.0f;
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f, ad = 0.0f;   // aw, ad: AUX only
  for (long s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float t = 0.0f, d = 0.0f;
    if (act) {
      if (COMPACT) {
        const half4 c16 = reinterpret_cast<const half4*>(radiance)[base + s0 + lane];
        c = make_float4(__half2float(c16.x), __half2float(c16.y), __half2float(c16.z), __half2float(c16.w));
        if (MODE == RTXN_VR_COMPAT) t = (float)((int)((s0 + lane) % K) + 1) * (1.0f / (float)K);
        else t = ray_hit[(base + s0 + lane) / K];       // compact NERF: one step length per SEGMENT
      } else {
        c = radiance[base + s0 + lane];
        t = ray_hit[base + s0 + lane];
      }
      if constexpr (AUX) {
        if (want_depth) {
          const long j = seg + (s0 + lane) / K;
          const float ts = aux.t_start[j], te = aux.t_end[j];
          d = fmaf(((float)((s0 + lane) % K) + aux.u0) * (1.0f / (float)K), te - ts, ts);
        }
      }
    }
    float x, w;
    if (MODE == RTXN_VR_COMPAT) {
      float tp = lane_below(t);
      if (lane == 0) tp = t_carry;
      const float delta = fabsf(t - tp);
      x = act ? delta * c.w : 0.0f;
      const float T = T_carry + wave_incl_scan_f(x);
      w = act ? expf(-T) * (1.0f - expf(-x)) : 0.0f;
      T_carry = lane63(T);
      // last ACTIVE lane's t carries over; inactive lanes only occur in the final step
      t_carry = lane63(t);
    } else {
      x = act ? t * c.w : 0.0f;  // ray_hit = step length
      const float incl = wave_incl_scan_f(x);
      const float T_excl = T_carry + incl - x;
      w = act ? expf(-T_excl) * (1.0f - expf(-x)) : 0.0f;
      T_carry += lane63(incl);
    }
    ar = fmaf(w, c.x, ar);
    ag = fmaf(w, c.y, ag);
    ab = fmaf(w, c.z, ab);
    if constexpr (AUX) {
      aw += w;
      ad = fmaf(w, d, ad);
    }
  }
  ar = wave_sum(ar);
  ag = wave_sum(ag);
  ab = wave_sum(ab);
  if constexpr (AUX) {
    aw = wave_sum(aw);
    if (want_depth) ad = wave_sum(ad);
  }
  if (lane == 0) {
    if constexpr (AUX) {
      const float rest = 1.0f - aw;
      if (aux.bg[0] != 0.0f) ar = fmaf(rest, aux.bg[0], ar);
      if (aux.bg[1] != 0.0f) ag = fmaf(rest, aux.bg[1], ag);
      if (aux.bg[2] != 0.0f) ab = fmaf(rest, aux.bg[2], ab);
    }
    pixels[3 * (long)ray] = ar;
    pixels[3 * (long)ray + 1] = ag;
    pixels[3 * (long)ray + 2] = ab;
    if constexpr (AUX) {
      if (aux.opacity) aux.opacity[ray] = aw;
      if (want_depth) aux.depth[ray] = ad;
    }
  }
}
template <int MODE, bool COMPACT = false>
__global__ __launch_bounds__(256) void volrender_fwd_kernel(const float4* __restrict__ radiance,
                                                            const int* __restrict__ num_hits,
                                                            const int* __restrict__ indices,
                                                            const float* __restrict__ ray_hit, int batch_size, int K,
                                                            float* __restrict__ pixels) {
  fwd_body<MODE, COMPACT, false>(radiance, num_hits, indices, ray_hit, batch_size, K, pixels, AuxArgs{});
}
template <int MODE, bool COMPACT>
__global__ __launch_bounds__(256) void volrender_aux_kernel(const float4* __restrict__ radiance,
                                                            const int* __restrict__ num_hits,
                                                            const int* __restrict__ indices,
                                                            const float* __restrict__ ray_hit, int batch_size, int K,
                                                            float* __restrict__ pixels, AuxArgs aux) {
  fwd_body<MODE, COMPACT, true>(radiance, num_hits, indices, ray_hit, batch_size, K, pixels, aux);
}

// Two samples per lane, 128 per step, and the next step's loads in flight while this step is scanned.  The one-sample form
// above has ONE 8/16-byte load outstanding per lane at a time and a serial dependence from step to step (the carried optical
// depth): measured 2.5 TB/s on the compact half4 radiance (0.31 of HBM).  Here a wave instruction moves 1 KiB (compact) or
// 2 x 1 KiB + 512 B (float4 + t) and two steps' worth is outstanding.  Needs an even K (pairs never straddle a ray's end and
// the 16-byte loads stay aligned); the arithmetic is the same for the compact and the float4 form, so their pixels remain
// bit-identical to each other.
// A wave takes kRaysPerWave CONSECUTIVE rays one after the other: 70 % of the bench frame's rays cross no occupied cell, and
// with a wave per ray the launch was bound by wave turnover (640 k waves, most of them exiting at once), not by HBM.
constexpr int kRaysPerWave = 4;

template <int MODE, bool COMPACT>
__global__ __launch_bounds__(256) void volrender_fwd_pair_kernel(const float4* __restrict__ radiance,
                                                                 const int* __restrict__ num_hits,
                                                                 const int* __restrict__ indices,
                                                                 const float* __restrict__ ray_hit, int batch_size, int K,
                                                                 float* __restrict__ pixels) {
  const int lane = threadIdx.x & 63;
  const int ray0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * kRaysPerWave;
  if (ray0 >= batch_size) return;
  const float rK = 1.0f / (float)K;
  struct Pair { float4 c0, c1; float t0, t1; };
  // per-ray CSR records of the wave's rays, fetched together up front (lanes 0..kRaysPerWave-1)
  const int my = ray0 + lane < batch_size && lane < kRaysPerWave ? ray0 + lane : ray0;
  const int idx_l = indices[my], nh_l = num_hits[my];
  float out = 0.0f;                                   // lane 3 r + ch of the wave holds pixel channel ch of ray r
  // sample counts of one ray fit 32 bits (<= 3R segments x K); only the ray's base offset is 64-bit.  K is a power of two in
  // every configuration of the reference (32): the index within the segment is then a mask, not a division.
  const int kmask = (K & (K - 1)) == 0 ? K - 1 : 0;
  const int kshift = kmask ? __builtin_ctz((unsigned)K) : 0;
  auto load = [&](long base, long seg0, int n, int s0, Pair& p) {
    const int i0 = s0 + 2 * lane;
    p.c0 = p.c1 = make_float4(0.f, 0.f, 0.f, 0.f);
    p.t0 = p.t1 = 0.0f;
    if (i0 < n) {
      if (COMPACT) {
        const uint4 raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const half4*>(radiance) + base + i0);   // two half4
        const __half2 a = *reinterpret_cast<const __half2*>(&raw.x), b = *reinterpret_cast<const __half2*>(&raw.y);
        const __half2 c = *reinterpret_cast<const __half2*>(&raw.z), d = *reinterpret_cast<const __half2*>(&raw.w);
        p.c0 = make_float4(__low2float(a), __high2float(a), __low2float(b), __high2float(b));
        p.c1 = make_float4(__low2float(c), __high2float(c), __low2float(d), __high2float(d));
        if (MODE == RTXN_VR_COMPAT) {
          // REGULAR t_vals (sampler.cu:52-66): (i + 1) / K of the index in the segment; i0 is even and K even: no wrap inside a pair
          const int k0 = kmask ? (i0 & kmask) : i0 % K;
          p.t0 = (float)(k0 + 1) * rK;
          p.t1 = (float)(k0 + 2) * rK;
        } else {
          p.t0 = p.t1 = ray_hit[seg0 + (kmask ? i0 >> kshift : i0 / K)];   // the segment's step length (a pair never straddles two)
        }
      } else {
        p.c0 = radiance[base + i0];
        p.c1 = radiance[base + i0 + 1];
        const float2 tt = *reinterpret_cast<const float2*>(ray_hit + base + i0);
        p.t0 = tt.x;
        p.t1 = tt.y;
      }
    }
  };
  // The frame has few samples per ray (70 % of the bench frame's rays have none, the rest ~500), so a wave's time is its
  // chain of dependent memory round trips: the first step of ALL its rays is requested before any ray is composited.
  long base_r[kRaysPerWave], seg_r[kRaysPerWave];
  int n_r[kRaysPerWave];
  Pair first[kRaysPerWave];
#pragma unroll
  for (int r = 0; r < kRaysPerWave; ++r) {
    seg_r[r] = (long)__shfl(idx_l, r, 64);
    base_r[r] = seg_r[r] * K;
    n_r[r] = ray0 + r < batch_size ? __shfl(nh_l, r, 64) * K : 0;     // even
    if (n_r[r] > 0) load(base_r[r], seg_r[r], n_r[r], 0, first[r]);
  }
#pragma unroll
  for (int r = 0; r < kRaysPerWave; ++r) {
    if (ray0 + r >= batch_size) break;
    const long base = base_r[r];
    const int n = n_r[r];
    float T_carry = 0.0f, t_carry = 0.0f;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    Pair cur = first[r], nxt;
    for (int s0 = 0; s0 < n; s0 += 128) {
      if (s0 + 128 < n) load(base, seg_r[r], n, s0 + 128, nxt);          // in flight under this step's scan
      const bool act = s0 + 2 * lane < n;
      float x0, x1, w0, w1;
      if (MODE == RTXN_VR_COMPAT) {
        float tp = lane_below(cur.t1);          // previous sample's t: the neighbour lane's second sample
        if (lane == 0) tp = t_carry;
        x0 = act ? fabsf(cur.t0 - tp) * cur.c0.w : 0.0f;
        x1 = act ? fabsf(cur.t1 - cur.t0) * cur.c1.w : 0.0f;
        const float pr = x0 + x1;
        const float T0 = (T_carry + (wave_incl_scan_f(pr) - pr)) + x0;   // inclusive optical depth at sample 0 of the pair
        const float T1 = T0 + x1;
        // three hardware exponentials per pair (v_exp_f32 on x log2 e; exp(-T1) = exp(-T0) exp(-x1)) instead of four libm
        // expf of ~12 instructions each: the compact form of this kernel is bound by its instruction count, not by HBM
        const float e0 = __expf(-T0), ex0 = __expf(-x0), ex1 = __expf(-x1);
        w0 = act ? e0 * (1.0f - ex0) : 0.0f;
        w1 = act ? (e0 * ex1) * (1.0f - ex1) : 0.0f;
        T_carry = lane63(T1);
        t_carry = lane63(cur.t1);             // inactive lanes only occur in the final step
      } else {
        x0 = act ? cur.t0 * cur.c0.w : 0.0f;          // ray_hit = step length
        x1 = act ? cur.t1 * cur.c1.w : 0.0f;
        const float pr = x0 + x1;
        const float incl = wave_incl_scan_f(pr);
        const float T0 = T_carry + (incl - pr);       // exclusive transmittance exponent of sample 0
        const float e0 = __expf(-T0), ex0 = __expf(-x0), ex1 = __expf(-x1);
        w0 = act ? e0 * (1.0f - ex0) : 0.0f;
        w1 = act ? (e0 * ex0) * (1.0f - ex1) : 0.0f;
        T_carry += lane63(incl);
      }
      ar = fmaf(w1, cur.c1.x, fmaf(w0, cur.c0.x, ar));
      ag = fmaf(w1, cur.c1.y, fmaf(w0, cur.c0.y, ag));
      ab = fmaf(w1, cur.c1.z, fmaf(w0, cur.c0.z, ab));
      cur = nxt;
    }
    if (n > 0) {                                      // wave-uniform
      ar = wave_sum(ar);
      ag = wave_sum(ag);
      ab = wave_sum(ab);
    }
    if (lane == 3 * r) out = ar;
    if (lane == 3 * r + 1) out = ag;
    if (lane == 3 * r + 2) out = ab;
  }
  // the wave's pixels are 3 * kRaysPerWave consecutive floats: one store
  if (lane < 3 * kRaysPerWave && ray0 + lane / 3 < batch_size) pixels[3 * (long)ray0 + lane] = out;
}

// COMPAT backward: per-sample, reference vol_render.cu:75-143 (not the analytic
// gradient of the forward).
__global__ __launch_bounds__(256) void volrender_bwd_compat_kernel(const __half* __restrict__ loss_gradients,
                                                                   const float4* __restrict__ radiance,
                                                                   const float* __restrict__ t_hit,
                                                                   const int* __restrict__ num_hits,
                                                                   const int* __restrict__ indices, int batch_size,
                                                                   int K, half4* __restrict__ grads) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= batch_size) return;
  const long base = (long)indices[ray] * K;
  const long n = (long)num_hits[ray] * K;
  const float g0 = __half2float(loss_gradients[3 * (long)ray]);
  const float g1 = __half2float(loss_gradients[3 * (long)ray + 1]);
  const float g2 = __half2float(loss_gradients[3 * (long)ray + 2]);
  float t_carry = 0.0f;
  for (long s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float t = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      t = t_hit[base + s0 + lane];
    }
    float tp = lane_below(t);
    if (lane == 0) tp = t_carry;
    t_carry = lane63(t);
    if (act) {
      const float delta = fabsf(t - tp);
      const float sigma = c.w;
      const float tr = delta * sigma;
      const float e = expf(-sigma * delta);
      float dg = 0.0f;
      dg += g0 * tr * c.x * delta * e;
      dg += g1 * tr * c.y * delta * e;
      dg += g2 * tr * c.z * delta * e;
      const float om = 1.0f - expf(-delta * sigma);
      half4 o;
      o.x = __float2half(g0 * tr * om);
      o.y = __float2half(g1 * tr * om);
      o.z = __float2half(g2 * tr * om);
      o.w = __float2half(dg);
      grads[base + s0 + lane] = o;
    }
  }
}

// NERF backward: exact gradient of the RTXN_VR_NERF forward.
//   C = sum_i T_i a_i c_i,  a_i = 1 - exp(-x_i), x_i = d_i sigma_i, T_i = exp(-sum_{k<i} x_k)
//   dC/dc_i = T_i a_i ;  dC/dsigma_i = d_i ( T_i exp(-x_i) c_i  -  sum_{k>i} T_k a_k c_k )   (per channel, dotted with g)
// Two sweeps per ray: forward sweep accumulates the total S = sum_k w_k (g.c_k); the
// per-sample suffix is S - inclusive_prefix.
__global__ __launch_bounds__(256) void volrender_bwd_nerf_kernel(const __half* __restrict__ loss_gradients,
                                                                 const float4* __restrict__ radiance,
                                                                 const float* __restrict__ step_len,
                                                                 const int* __restrict__ num_hits,
                                                                 const int* __restrict__ indices, int batch_size,
                                                                 int K, half4* __restrict__ grads) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= batch_size) return;
  const long base = (long)indices[ray] * K;
  const long n = (long)num_hits[ray] * K;
  const float g0 = __half2float(loss_gradients[3 * (long)ray]);
  const float g1 = __half2float(loss_gradients[3 * (long)ray + 1]);
  const float g2 = __half2float(loss_gradients[3 * (long)ray + 2]);
  // sweep 1: S = sum_k w_k (g . c_k)
  float T_carry = 0.0f, S = 0.0f;
  for (long s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float d = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      d = step_len[base + s0 + lane];
    }
    const float x = d * c.w;
    const float incl = wave_incl_scan_f(x);
    const float w = expf(-(T_carry + incl - x)) * (1.0f - expf(-x));
    S += w * (g0 * c.x + g1 * c.y + g2 * c.z);
    T_carry += lane63(incl);
  }
  S = wave_sum(S);
  // sweep 2: per-sample gradients
  T_carry = 0.0f;
  float P_carry = 0.0f;  // inclusive prefix of w_k (g.c_k)
  for (long s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float d = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      d = step_len[base + s0 + lane];
    }
    const float x = d * c.w;
    const float incl = wave_incl_scan_f(x);
    const float Ti = expf(-(T_carry + incl - x));
    const float ex = expf(-x);
    const float a = 1.0f - ex;
    const float gc = g0 * c.x + g1 * c.y + g2 * c.z;
    const float wgc = Ti * a * gc;
    const float pincl = P_carry + wave_incl_scan_f(wgc);
    if (act) {
      const float suffix = S - pincl;
      half4 o;
      o.x = __float2half(g0 * Ti * a);
      o.y = __float2half(g1 * Ti * a);
      o.z = __float2half(g2 * Ti * a);
      o.w = __float2half(d * (Ti * ex * gc - suffix));
      grads[base + s0 + lane] = o;
    }
    T_carry += lane63(incl);
    P_carry = lane63(pincl);
  }
}

// launch_volrender_cuda + loss->evaluate (L2) + launch_volrender_backward_cuda of one training batch in ONE launch
// (RTXN_VR_NERF).  A ray's loss gradient depends on its own pixel only, and the first sweep of the exact backward --
// S = sum_k w_k (g . c_k) -- is the forward's pixel dotted with g, so the forward sweep serves both: sweep 1 composites the
// pixel, the wave forms d = pixel - target, the L2 value and g = half(loss_scale 2 d / n) (the fp16 rounding
// network->backward sees, main.cu:759), sweep 2 writes the per-sample gradients.  Three launches and one pass over the
// radiance fewer than the separate entry points; same arithmetic per sample (S differs by fp32 rounding: g . pixel
// instead of the per-sample sum).
__global__ __launch_bounds__(256) void volrender_l2_fused_kernel(const float4* __restrict__ radiance, const float* __restrict__ step_len,
                                                                 const int* __restrict__ num_hits, const int* __restrict__ indices,
                                                                 int batch_size, int K, const float* __restrict__ target,
                                                                 float loss_scale, float* __restrict__ pixels,
                                                                 __half* __restrict__ loss_gradients, float* __restrict__ loss_sum,
                                                                 half4* __restrict__ grads) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= batch_size) return;
  const long base = (long)indices[ray] * K;
  const long n = (long)num_hits[ray] * K;
  const float inv_n = 1.0f / (float)(3L * batch_size);
  // sweep 1: the pixel
  float T_carry = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
  for (long s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float d = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      d = step_len[base + s0 + lane];
    }
    const float x = d * c.w;
    const float incl = wave_incl_scan_f(x);
    const float w = act ? expf(-(T_carry + incl - x)) * (1.0f - expf(-x)) : 0.0f;
    ar = fmaf(w, c.x, ar);
    ag = fmaf(w, c.y, ag);
    ab = fmaf(w, c.z, ab);
    T_carry += lane63(incl);
  }
  ar = wave_sum(ar);
  ag = wave_sum(ag);
  ab = wave_sum(ab);
  // L2 (tcnn "L2": values = d^2 / n, gradients = loss_scale * 2 d / n, rounded to fp16)
  const float d0 = ar - target[3 * (long)ray], d1 = ag - target[3 * (long)ray + 1], d2 = ab - target[3 * (long)ray + 2];
  const __half h0 = __float2half(loss_scale * 2.0f * d0 * inv_n), h1 = __float2half(loss_scale * 2.0f * d1 * inv_n),
               h2 = __float2half(loss_scale * 2.0f * d2 * inv_n);
  const float g0 = __half2float(h0), g1 = __half2float(h1), g2 = __half2float(h2);
  if (lane == 0) {
    pixels[3 * (long)ray] = ar;
    pixels[3 * (long)ray + 1] = ag;
    pixels[3 * (long)ray + 2] = ab;
    if (loss_gradients) {
      loss_gradients[3 * (long)ray] = h0;
      loss_gradients[3 * (long)ray + 1] = h1;
      loss_gradients[3 * (long)ray + 2] = h2;
    }
    if (loss_sum) atomicAdd(loss_sum, (d0 * d0 + d1 * d1 + d2 * d2) * inv_n);
  }
  const float S = g0 * ar + g1 * ag + g2 * ab;     // = sum_k w_k (g . c_k)
  // sweep 2: per-sample gradients (volrender_bwd_nerf_kernel's second sweep)
  T_carry = 0.0f;
  float P_carry = 0.0f;
  for (long s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float d = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      d = step_len[base + s0 + lane];
    }
    const float x = d * c.w;
    const float incl = wave_incl_scan_f(x);
    const float Ti = expf(-(T_carry + incl - x));
    const float ex = expf(-x);
    const float a = 1.0f - ex;
    const float gc = g0 * c.x + g1 * c.y + g2 * c.z;
    const float wgc = Ti * a * gc;
    const float pincl = P_carry + wave_incl_scan_f(wgc);
    if (act) {
      const float suffix = S - pincl;
      half4 o;
      o.x = __float2half(g0 * Ti * a);
      o.y = __float2half(g1 * Ti * a);
      o.z = __float2half(g2 * Ti * a);
      o.w = __float2half(d * (Ti * ex * gc - suffix));
      grads[base + s0 + lane] = o;
    }
    T_carry += lane63(incl);
    P_carry = lane63(pincl);
  }
}

// The training compositor as it runs by default: U blocks of 128 samples (two adjacent samples per lane) per step, their scans
// independent and interleaved, the block offsets chained through scalar registers.  A training batch has few, long rays (the
// configs[2] batch: 12 % of the 4096 rays hit anything, those cross 44 occupied cells on average and up to 128 = 4096
// samples), so the launch lasts as long as the LONGEST ray's chain of dependent steps: 512 samples per step make that 8
// steps per sweep instead of 32.  The loss is reduced per block and added ONCE per block at the very end: a same-address
// atomic per ray sat in front of the second sweep's loads in every wave's in-order memory counter (+45 us of 91).
template <int U>
__global__ __launch_bounds__(256) void volrender_l2_fused_multi_kernel(const float4* __restrict__ radiance, const float* __restrict__ step_len,
                                                                       const int* __restrict__ num_hits, const int* __restrict__ indices,
                                                                       int batch_size, int K, const float* __restrict__ target,
                                                                       float loss_scale, float* __restrict__ pixels,
                                                                       __half* __restrict__ loss_gradients, float* __restrict__ loss_sum,
                                                                       half4* __restrict__ grads) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ray = blockIdx.x * 4 + wave;
  float loss_part = 0.0f;
  if (ray < batch_size) {
    const long base = (long)indices[ray] * K;
    const long n = (long)num_hits[ray] * K;          // even
    const float inv_n = 1.0f / (float)(3L * batch_size);
    constexpr long STEP = 128L * U;
    struct Pair { float4 c0, c1; float d0, d1; };
    auto load = [&](long s0, Pair (&p)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long i0 = s0 + 128 * u + 2 * lane;
        p[u].c0 = p[u].c1 = make_float4(0.f, 0.f, 0.f, 0.f);
        p[u].d0 = p[u].d1 = 0.0f;
        if (i0 < n) {
          p[u].c0 = radiance[base + i0];
          p[u].c1 = radiance[base + i0 + 1];
          const float2 dd = *reinterpret_cast<const float2*>(step_len + base + i0);
          p[u].d0 = dd.x;
          p[u].d1 = dd.y;
        }
      }
    };
    // sweep 1: the pixel
    float T_carry = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
    Pair cur[U], nxt[U];
    if (n > 0) load(0, cur);
    for (long s0 = 0; s0 < n; s0 += STEP) {
      if (s0 + STEP < n) load(s0 + STEP, nxt);
      float x0[U], x1[U], pr[U], incl[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x0[u] = cur[u].d0 * cur[u].c0.w;                 // inactive lanes hold zeros: x = 0, w = 0
        x1[u] = cur[u].d1 * cur[u].c1.w;
        pr[u] = x0[u] + x1[u];
        incl[u] = wave_incl_scan_f(pr[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float T0 = T_carry + (incl[u] - pr[u]);
        const float w0 = expf(-T0) * (1.0f - expf(-x0[u])), w1 = expf(-(T0 + x0[u])) * (1.0f - expf(-x1[u]));
        ar = fmaf(w1, cur[u].c1.x, fmaf(w0, cur[u].c0.x, ar));
        ag = fmaf(w1, cur[u].c1.y, fmaf(w0, cur[u].c0.y, ag));
        ab = fmaf(w1, cur[u].c1.z, fmaf(w0, cur[u].c0.z, ab));
        T_carry += lane63(incl[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
    ar = wave_sum(ar);
    ag = wave_sum(ag);
    ab = wave_sum(ab);
    float g0, g1, g2;
    if (target) {
      const float e0 = ar - target[3 * (long)ray], e1 = ag - target[3 * (long)ray + 1], e2 = ab - target[3 * (long)ray + 2];
      const __half h0 = __float2half(loss_scale * 2.0f * e0 * inv_n), h1 = __float2half(loss_scale * 2.0f * e1 * inv_n),
                   h2 = __float2half(loss_scale * 2.0f * e2 * inv_n);
      g0 = __half2float(h0); g1 = __half2float(h1); g2 = __half2float(h2);
      if (lane == 0) {
        pixels[3 * (long)ray] = ar;
        pixels[3 * (long)ray + 1] = ag;
        pixels[3 * (long)ray + 2] = ab;
        if (loss_gradients) {
          loss_gradients[3 * (long)ray] = h0;
          loss_gradients[3 * (long)ray + 1] = h1;
          loss_gradients[3 * (long)ray + 2] = h2;
        }
      }
      loss_part = (e0 * e0 + e1 * e1 + e2 * e2) * inv_n;
    } else {      // rtxn_volrender_bwd: the pixel gradients are given (launch_volrender_backward_cuda's loss_gradients)
      g0 = __half2float(loss_gradients[3 * (long)ray]);
      g1 = __half2float(loss_gradients[3 * (long)ray + 1]);
      g2 = __half2float(loss_gradients[3 * (long)ray + 2]);
    }
    const float S = g0 * ar + g1 * ag + g2 * ab;
    // sweep 2: per-sample gradients (the radiance is re-read: cache hits)
    T_carry = 0.0f;
    float P_carry = 0.0f;
    if (n > 0) load(0, cur);
    for (long s0 = 0; s0 < n; s0 += STEP) {
      if (s0 + STEP < n) load(s0 + STEP, nxt);
      float x0[U], x1[U], pr[U], incl[U], T0[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x0[u] = cur[u].d0 * cur[u].c0.w;
        x1[u] = cur[u].d1 * cur[u].c1.w;
        pr[u] = x0[u] + x1[u];
        incl[u] = wave_incl_scan_f(pr[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        T0[u] = T_carry + (incl[u] - pr[u]);
        T_carry += lane63(incl[u]);
      }
      float Ti0[U], Ti1[U], ex0[U], ex1[U], gc0[U], gc1[U], wgc1[U], pin[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        Ti0[u] = expf(-T0[u]);
        Ti1[u] = expf(-(T0[u] + x0[u]));
        ex0[u] = expf(-x0[u]);
        ex1[u] = expf(-x1[u]);
        gc0[u] = g0 * cur[u].c0.x + g1 * cur[u].c0.y + g2 * cur[u].c0.z;
        gc1[u] = g0 * cur[u].c1.x + g1 * cur[u].c1.y + g2 * cur[u].c1.z;
        const float wgc0 = Ti0[u] * (1.0f - ex0[u]) * gc0[u];
        wgc1[u] = Ti1[u] * (1.0f - ex1[u]) * gc1[u];
        pin[u] = wave_incl_scan_f(wgc0 + wgc1[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long i0 = s0 + 128 * u + 2 * lane;
        const float pincl1 = P_carry + pin[u];          // inclusive prefix at the pair's second sample
        const float pincl0 = pincl1 - wgc1[u];
        P_carry += lane63(pin[u]);
        if (i0 < n) {
          const float a0 = 1.0f - ex0[u], a1 = 1.0f - ex1[u];
          half4 o0, o1;
          o0.x = __float2half(g0 * Ti0[u] * a0);
          o0.y = __float2half(g1 * Ti0[u] * a0);
          o0.z = __float2half(g2 * Ti0[u] * a0);
          o0.w = __float2half(cur[u].d0 * (Ti0[u] * ex0[u] * gc0[u] - (S - pincl0)));
          o1.x = __float2half(g0 * Ti1[u] * a1);
          o1.y = __float2half(g1 * Ti1[u] * a1);
          o1.z = __float2half(g2 * Ti1[u] * a1);
          o1.w = __float2half(cur[u].d1 * (Ti1[u] * ex1[u] * gc1[u] - (S - pincl1)));
          uint4 packed;
          packed.x = *reinterpret_cast<const unsigned*>(&o0.x);
          packed.y = *reinterpret_cast<const unsigned*>(&o0.z);
          packed.z = *reinterpret_cast<const unsigned*>(&o1.x);
          packed.w = *reinterpret_cast<const unsigned*>(&o1.z);
          *reinterpret_cast<uint4*>(grads + base + i0) = packed;      // two half4: one 16-byte store
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
  }
  if (loss_sum) {
    if (lane == 0) red[wave] = loss_part;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss_sum, (red[0] + red[1]) + (red[2] + red[3]));
  }
}

template <int MODE, bool COMPACT>
__global__ __launch_bounds__(256) void volrender_aux_pair_kernel(const float4* __restrict__ radiance,
                                                                 const int* __restrict__ num_hits,
                                                                 const int* __restrict__ indices,
                                                                 const float* __restrict__ ray_hit, int batch_size, int K,
                                                                 float* __restrict__ pixels, AuxArgs aux) {
  const int lane = threadIdx.x & 63;
  const int ray0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * kRaysPerWave;
  if (ray0 >= batch_size) return;
  const float rK = 1.0f / (float)K;
  const bool want_depth = aux.depth != nullptr;
  struct Pair { float4 c0, c1; float t0, t1, d0, d1; };
  const int my = ray0 + lane < batch_size && lane < kRaysPerWave ? ray0 + lane : ray0;
  const int idx_l = indices[my], nh_l = num_hits[my];
  float out = 0.0f;                                   // lane 3 r + ch: pixel channel ch of ray r
  float out_a = 0.0f;                                 // lanes 3 r .. 3 r + 2: opacity of ray r (the background's weight)
  float out_o = 0.0f, out_d = 0.0f;                   // lane r: opacity and depth of ray r
  const int kmask = (K & (K - 1)) == 0 ? K - 1 : 0;
  const int kshift = kmask ? __builtin_ctz((unsigned)K) : 0;
  auto load = [&](long base, long seg0, int n, int s0, Pair& p) {
    const int i0 = s0 + 2 * lane;
    p.c0 = p.c1 = make_float4(0.f, 0.f, 0.f, 0.f);
    p.t0 = p.t1 = p.d0 = p.d1 = 0.0f;
    if (i0 < n) {
      const int j = kmask ? i0 >> kshift : i0 / K;          // a pair never straddles two segments (K even)
      if (COMPACT) {
        const uint4 raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const half4*>(radiance) + base + i0);
        const __half2 a = *reinterpret_cast<const __half2*>(&raw.x), b = *reinterpret_cast<const __half2*>(&raw.y);
        const __half2 c = *reinterpret_cast<const __half2*>(&raw.z), d = *reinterpret_cast<const __half2*>(&raw.w);
        p.c0 = make_float4(__low2float(a), __high2float(a), __low2float(b), __high2float(b));
        p.c1 = make_float4(__low2float(c), __high2float(c), __low2float(d), __high2float(d));
        if (MODE == RTXN_VR_COMPAT) {
          const int k0 = kmask ? (i0 & kmask) : i0 % K;
          p.t0 = (float)(k0 + 1) * rK;
          p.t1 = (float)(k0 + 2) * rK;
        } else {
          p.t0 = p.t1 = ray_hit[seg0 + j];
        }
      } else {
        p.c0 = radiance[base + i0];
        p.c1 = radiance[base + i0 + 1];
        const float2 tt = *reinterpret_cast<const float2*>(ray_hit + base + i0);
        p.t0 = tt.x;
        p.t1 = tt.y;
      }
      if (want_depth) {
        const int k0 = kmask ? (i0 & kmask) : i0 % K;
        const float ts = aux.t_start[seg0 + j], len = aux.t_end[seg0 + j] - ts;
        p.d0 = fmaf(((float)k0 + aux.u0) * rK, len, ts);
        p.d1 = fmaf(((float)(k0 + 1) + aux.u0) * rK, len, ts);
      }
    }
  };
  long base_r[kRaysPerWave], seg_r[kRaysPerWave];
  int n_r[kRaysPerWave];
  Pair first[kRaysPerWave];
#pragma unroll
  for (int r = 0; r < kRaysPerWave; ++r) {
    seg_r[r] = (long)__shfl(idx_l, r, 64);
    base_r[r] = seg_r[r] * K;
    n_r[r] = ray0 + r < batch_size ? __shfl(nh_l, r, 64) * K : 0;
    if (n_r[r] > 0) load(base_r[r], seg_r[r], n_r[r], 0, first[r]);
  }
#pragma unroll
  for (int r = 0; r < kRaysPerWave; ++r) {
    if (ray0 + r >= batch_size) break;
    const long base = base_r[r];
    const int n = n_r[r];
    float T_carry = 0.0f, t_carry = 0.0f;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f, ad = 0.0f;
    Pair cur = first[r], nxt;
    for (int s0 = 0; s0 < n; s0 += 128) {
      if (s0 + 128 < n) load(base, seg_r[r], n, s0 + 128, nxt);
      const bool act = s0 + 2 * lane < n;
      float x0, x1, w0, w1;
      if (MODE == RTXN_VR_COMPAT) {
        float tp = lane_below(cur.t1);
        if (lane == 0) tp = t_carry;
        x0 = act ? fabsf(cur.t0 - tp) * cur.c0.w : 0.0f;
        x1 = act ? fabsf(cur.t1 - cur.t0) * cur.c1.w : 0.0f;
        const float pr = x0 + x1;
        const float T0 = (T_carry + (wave_incl_scan_f(pr) - pr)) + x0;
        const float T1 = T0 + x1;
        const float e0 = __expf(-T0), ex0 = __expf(-x0), ex1 = __expf(-x1);
        w0 = act ? e0 * (1.0f - ex0) : 0.0f;
        w1 = act ? (e0 * ex1) * (1.0f - ex1) : 0.0f;
        T_carry = lane63(T1);
        t_carry = lane63(cur.t1);
      } else {
        x0 = act ? cur.t0 * cur.c0.w : 0.0f;
        x1 = act ? cur.t1 * cur.c1.w : 0.0f;
        const float pr = x0 + x1;
        const float incl = wave_incl_scan_f(pr);
        const float T0 = T_carry + (incl - pr);
        const float e0 = __expf(-T0), ex0 = __expf(-x0), ex1 = __expf(-x1);
        w0 = act ? e0 * (1.0f - ex0) : 0.0f;
        w1 = act ? (e0 * ex0) * (1.0f - ex1) : 0.0f;
        T_carry += lane63(incl);
      }
      ar = fmaf(w1, cur.c1.x, fmaf(w0, cur.c0.x, ar));
      ag = fmaf(w1, cur.c1.y, fmaf(w0, cur.c0.y, ag));
      ab = fmaf(w1, cur.c1.z, fmaf(w0, cur.c0.z, ab));
      aw += w0 + w1;
      ad = fmaf(w1, cur.d1, fmaf(w0, cur.d0, ad));
      cur = nxt;
    }
    if (n > 0) {                                      // wave-uniform
      ar = wave_sum(ar);
      ag = wave_sum(ag);
      ab = wave_sum(ab);
      aw = wave_sum(aw);
      if (want_depth) ad = wave_sum(ad);
    }
    if (lane == 3 * r) out = ar;
    if (lane == 3 * r + 1) out = ag;
    if (lane == 3 * r + 2) out = ab;
    if (lane / 3 == r) out_a = aw;
    if (lane == r) {
      out_o = aw;
      out_d = ad;
    }
  }
  if (lane < 3 * kRaysPerWave && ray0 + lane / 3 < batch_size) {
    const int ch = lane - 3 * (lane / 3);
    const float bg = ch == 0 ? aux.bg[0] : ch == 1 ? aux.bg[1] : aux.bg[2];
    if (bg != 0.0f) out = fmaf(1.0f - out_a, bg, out);
    pixels[3 * (long)ray0 + lane] = out;
  }
  if (lane < kRaysPerWave && ray0 + lane < batch_size) {
    if (aux.opacity) aux.opacity[ray0 + lane] = out_o;
    if (want_depth) aux.depth[ray0 + lane] = out_d;
  }
}

// The training compositor over a background (rtxn_volrender_l2_train_ex): pixel = sum w c + (1 - A) bg with
// A = sum w.  Written as bg + sum w_k (c_k - bg) it is the plain compositor with colours c_k - bg: dL/dc_i is unchanged, the
// optical-depth gradient dots g with c_k - bg, and the second sweep's total is S' = g . (sum w c) - (g . bg) A.  Separate
// kernels beside the plain ones (copies with the additions written in: a shared inlined body changes the plain kernels' bytes).
// BgArgs and ray_background (the ray's background and composited target): background_internal.h, shared with loss.hip.

// one ray per wave, 64 samples per step: the form for odd K or misaligned buffers (volrender_l2_fused_kernel's arithmetic)
__global__ __launch_bounds__(256) void volrender_l2_bg_kernel(const float4* __restrict__ radiance, const float* __restrict__ step_len,
                                                              const int* __restrict__ num_hits, const int* __restrict__ indices,
                                                              int batch_size, int K, const float* __restrict__ target,
                                                              float loss_scale, float* __restrict__ pixels,
                                                              __half* __restrict__ loss_gradients, float* __restrict__ loss_sum,
                                                              half4* __restrict__ grads, BgArgs bga) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= batch_size) return;
  const long base = (long)indices[ray] * K;
  const long n = (long)num_hits[ray] * K;
  const float inv_n = 1.0f / (float)(3L * batch_size);
  float bg[3], tg[3];
  ray_background(bga, target, ray, bg, tg);
  // sweep 1: colour and opacity sums
  float T_carry = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f;
  for (long s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float d = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      d = step_len[base + s0 + lane];
    }
    const float x = d * c.w;
    const float incl = wave_incl_scan_f(x);
    const float w = act ? expf(-(T_carry + incl - x)) * (1.0f - expf(-x)) : 0.0f;
    ar = fmaf(w, c.x, ar);
    ag = fmaf(w, c.y, ag);
    ab = fmaf(w, c.z, ab);
    aw += w;
    T_carry += lane63(incl);
  }
  ar = wave_sum(ar);
  ag = wave_sum(ag);
  ab = wave_sum(ab);
  aw = wave_sum(aw);
  const float rest = 1.0f - aw;
  const float pr = fmaf(rest, bg[0], ar), pg = fmaf(rest, bg[1], ag), pb = fmaf(rest, bg[2], ab);
  const float d0 = pr - tg[0], d1 = pg - tg[1], d2 = pb - tg[2];
  const __half h0 = __float2half(loss_scale * 2.0f * d0 * inv_n), h1 = __float2half(loss_scale * 2.0f * d1 * inv_n),
               h2 = __float2half(loss_scale * 2.0f * d2 * inv_n);
  const float g0 = __half2float(h0), g1 = __half2float(h1), g2 = __half2float(h2);
  if (lane == 0) {
    pixels[3 * (long)ray] = pr;
    pixels[3 * (long)ray + 1] = pg;
    pixels[3 * (long)ray + 2] = pb;
    if (loss_gradients) {
      loss_gradients[3 * (long)ray] = h0;
      loss_gradients[3 * (long)ray + 1] = h1;
      loss_gradients[3 * (long)ray + 2] = h2;
    }
    if (loss_sum) atomicAdd(loss_sum, (d0 * d0 + d1 * d1 + d2 * d2) * inv_n);
  }
  const float gbg = g0 * bg[0] + g1 * bg[1] + g2 * bg[2];
  const float S = (g0 * ar + g1 * ag + g2 * ab) - gbg * aw;     // = sum_k w_k (g . (c_k - bg))
  // sweep 2: per-sample gradients
  T_carry = 0.0f;
  float P_carry = 0.0f;
  for (long s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float d = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      d = step_len[base + s0 + lane];
    }
    const float x = d * c.w;
    const float incl = wave_incl_scan_f(x);
    const float Ti = expf(-(T_carry + incl - x));
    const float ex = expf(-x);
    const float a = 1.0f - ex;
    const float gc = (g0 * c.x + g1 * c.y + g2 * c.z) - gbg;
    const float wgc = act ? Ti * a * gc : 0.0f;
    const float pincl = P_carry + wave_incl_scan_f(wgc);
    if (act) {
      const float suffix = S - pincl;
      half4 o;
      o.x = __float2half(g0 * Ti * a);
      o.y = __float2half(g1 * Ti * a);
      o.z = __float2half(g2 * Ti * a);
      o.w = __float2half(d * (Ti * ex * gc - suffix));
      grads[base + s0 + lane] = o;
    }
    T_carry += lane63(incl);
    P_carry = lane63(pincl);
  }
}

// U blocks of 128 samples per step, two per lane (volrender_l2_fused_multi_kernel's schedule and arithmetic, plus the opacity
// sum in sweep 1 and the background's dot product in sweep 2)
template <int U>
__global__ __launch_bounds__(256) void volrender_l2_bg_multi_kernel(const float4* __restrict__ radiance, const float* __restrict__ step_len,
                                                                    const int* __restrict__ num_hits, const int* __restrict__ indices,
                                                                    int batch_size, int K, const float* __restrict__ target,
                                                                    float loss_scale, float* __restrict__ pixels,
                                                                    __half* __restrict__ loss_gradients, float* __restrict__ loss_sum,
                                                                    half4* __restrict__ grads, BgArgs bga) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ray = blockIdx.x * 4 + wave;
  float loss_part = 0.0f;
  if (ray < batch_size) {
    const long base = (long)indices[ray] * K;
    const long n = (long)num_hits[ray] * K;          // even
    const float inv_n = 1.0f / (float)(3L * batch_size);
    float bg[3], tg[3];
    ray_background(bga, target, ray, bg, tg);
    constexpr long STEP = 128L * U;
    struct Pair { float4 c0, c1; float d0, d1; };
    auto load = [&](long s0, Pair (&p)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long i0 = s0 + 128 * u + 2 * lane;
        p[u].c0 = p[u].c1 = make_float4(0.f, 0.f, 0.f, 0.f);
        p[u].d0 = p[u].d1 = 0.0f;
        if (i0 < n) {
          p[u].c0 = radiance[base + i0];
          p[u].c1 = radiance[base + i0 + 1];
          const float2 dd = *reinterpret_cast<const float2*>(step_len + base + i0);
          p[u].d0 = dd.x;
          p[u].d1 = dd.y;
        }
      }
    };
    // sweep 1: colour and opacity sums
    float T_carry = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f;
    Pair cur[U], nxt[U];
    if (n > 0) load(0, cur);
    for (long s0 = 0; s0 < n; s0 += STEP) {
      if (s0 + STEP < n) load(s0 + STEP, nxt);
      float x0[U], x1[U], pr[U], incl[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x0[u] = cur[u].d0 * cur[u].c0.w;                 // inactive lanes hold zeros: x = 0, w = 0
        x1[u] = cur[u].d1 * cur[u].c1.w;
        pr[u] = x0[u] + x1[u];
        incl[u] = wave_incl_scan_f(pr[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float T0 = T_carry + (incl[u] - pr[u]);
        const float w0 = expf(-T0) * (1.0f - expf(-x0[u])), w1 = expf(-(T0 + x0[u])) * (1.0f - expf(-x1[u]));
        ar = fmaf(w1, cur[u].c1.x, fmaf(w0, cur[u].c0.x, ar));
        ag = fmaf(w1, cur[u].c1.y, fmaf(w0, cur[u].c0.y, ag));
        ab = fmaf(w1, cur[u].c1.z, fmaf(w0, cur[u].c0.z, ab));
        aw += w0 + w1;
        T_carry += lane63(incl[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
    ar = wave_sum(ar);
    ag = wave_sum(ag);
    ab = wave_sum(ab);
    aw = wave_sum(aw);
    const float rest = 1.0f - aw;
    const float pxr = fmaf(rest, bg[0], ar), pxg = fmaf(rest, bg[1], ag), pxb = fmaf(rest, bg[2], ab);
    const float e0 = pxr - tg[0], e1 = pxg - tg[1], e2 = pxb - tg[2];
    const __half h0 = __float2half(loss_scale * 2.0f * e0 * inv_n), h1 = __float2half(loss_scale * 2.0f * e1 * inv_n),
                 h2 = __float2half(loss_scale * 2.0f * e2 * inv_n);
    const float g0 = __half2float(h0), g1 = __half2float(h1), g2 = __half2float(h2);
    if (lane == 0) {
      pixels[3 * (long)ray] = pxr;
      pixels[3 * (long)ray + 1] = pxg;
      pixels[3 * (long)ray + 2] = pxb;
      if (loss_gradients) {
        loss_gradients[3 * (long)ray] = h0;
        loss_gradients[3 * (long)ray + 1] = h1;
        loss_gradients[3 * (long)ray + 2] = h2;
      }
    }
    loss_part = (e0 * e0 + e1 * e1 + e2 * e2) * inv_n;
    const float gbg = g0 * bg[0] + g1 * bg[1] + g2 * bg[2];
    const float S = (g0 * ar + g1 * ag + g2 * ab) - gbg * aw;     // = sum_k w_k (g . (c_k - bg))
    // sweep 2: per-sample gradients (the radiance is re-read: cache hits)
    T_carry = 0.0f;
    float P_carry = 0.0f;
    if (n > 0) load(0, cur);
    for (long s0 = 0; s0 < n; s0 += STEP) {
      if (s0 + STEP < n) load(s0 + STEP, nxt);
      float x0[U], x1[U], pr[U], incl[U], T0[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x0[u] = cur[u].d0 * cur[u].c0.w;
        x1[u] = cur[u].d1 * cur[u].c1.w;
        pr[u] = x0[u] + x1[u];
        incl[u] = wave_incl_scan_f(pr[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        T0[u] = T_carry + (incl[u] - pr[u]);
        T_carry += lane63(incl[u]);
      }
      float Ti0[U], Ti1[U], ex0[U], ex1[U], gc0[U], gc1[U], wgc1[U], pin[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        Ti0[u] = expf(-T0[u]);
        Ti1[u] = expf(-(T0[u] + x0[u]));
        ex0[u] = expf(-x0[u]);
        ex1[u] = expf(-x1[u]);
        gc0[u] = (g0 * cur[u].c0.x + g1 * cur[u].c0.y + g2 * cur[u].c0.z) - gbg;
        gc1[u] = (g0 * cur[u].c1.x + g1 * cur[u].c1.y + g2 * cur[u].c1.z) - gbg;
        // inactive lanes: Ti (1 - ex) = 0 (x = 0), so the -gbg of their zero colour adds nothing to the prefix
        const float wgc0 = Ti0[u] * (1.0f - ex0[u]) * gc0[u];
        wgc1[u] = Ti1[u] * (1.0f - ex1[u]) * gc1[u];
        pin[u] = wave_incl_scan_f(wgc0 + wgc1[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long i0 = s0 + 128 * u + 2 * lane;
        const float pincl1 = P_carry + pin[u];          // inclusive prefix at the pair's second sample
        const float pincl0 = pincl1 - wgc1[u];
        P_carry += lane63(pin[u]);
        if (i0 < n) {
          const float a0 = 1.0f - ex0[u], a1 = 1.0f - ex1[u];
          half4 o0, o1;
          o0.x = __float2half(g0 * Ti0[u] * a0);
          o0.y = __float2half(g1 * Ti0[u] * a0);
          o0.z = __float2half(g2 * Ti0[u] * a0);
          o0.w = __float2half(cur[u].d0 * (Ti0[u] * ex0[u] * gc0[u] - (S - pincl0)));
          o1.x = __float2half(g0 * Ti1[u] * a1);
          o1.y = __float2half(g1 * Ti1[u] * a1);
          o1.z = __float2half(g2 * Ti1[u] * a1);
          o1.w = __float2half(cur[u].d1 * (Ti1[u] * ex1[u] * gc1[u] - (S - pincl1)));
          uint4 packed;
          packed.x = *reinterpret_cast<const unsigned*>(&o0.x);
          packed.y = *reinterpret_cast<const unsigned*>(&o0.z);
          packed.z = *reinterpret_cast<const unsigned*>(&o1.x);
          packed.w = *reinterpret_cast<const unsigned*>(&o1.z);
          *reinterpret_cast<uint4*>(grads + base + i0) = packed;      // two half4: one 16-byte store
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
  }
  if (loss_sum) {
    if (lane == 0) red[wave] = loss_part;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss_sum, (red[0] + red[1]) + (red[2] + red[3]));
  }
}

}  // namespace

// The background rules of every _ex training entry point (include/rtxn.h), checked before any device is touched.  *active: a
// background is to be composited (NULL, or NONE with 3-channel targets, run exactly what the plain entry point runs).
int rtxn::check_train_background(const rtxn_train_background* bg, int vr_mode, const char* who, bool* active) {
  *active = false;
  if (!bg) return RTXN_OK;
  RTXN_REQUIRE(bg->mode == RTXN_BG_NONE || bg->mode == RTXN_BG_CONSTANT || bg->mode == RTXN_BG_RANDOM,
               "%s: unknown background mode %d", who, bg->mode);
  RTXN_REQUIRE(bg->target_channels == 3 || bg->target_channels == 4, "%s: target_channels = %d (3 or 4)", who, bg->target_channels);
  RTXN_REQUIRE(!(bg->mode == RTXN_BG_RANDOM && bg->target_channels == 3),
               "%s: a RANDOM background needs 4-channel (RGBA) targets: a 3-channel target cannot know the background", who);
  RTXN_REQUIRE(!(bg->mode == RTXN_BG_NONE && bg->target_channels == 4),
               "%s: 4-channel (RGBA) targets need a CONSTANT or RANDOM background to be composited over", who);
  *active = bg->mode != RTXN_BG_NONE;
  RTXN_REQUIRE(!(*active && vr_mode == RTXN_VR_COMPAT),
               "%s: a background needs the RTXN_VR_NERF compositor (RTXN_VR_COMPAT's backward is not the gradient of its forward)", who);
  return RTXN_OK;
}

namespace {

// The forward family's launch: every entry point's choice between the pair and the one-sample kernel (two samples per lane
// need an even K and loads that stay aligned: 16 bytes of half4 radiance, or 8 bytes of t_vals beside float4 radiance) and
// the instantiation for its mode and radiance layout.  aux == NULL: the plain kernels.  `who` names the entry point in
// errors, `what` the kernel in a launch failure.
int launch_fwd(const char* who, const char* what, const void* radiance, bool half, int mode, const float* ray_hit,
               const int* num_hits, const int* indices, int batch_size, int K, float* pixels, const AuxArgs* aux,
               rtxn_stream_t stream) {
  RTXN_REQUIRE(((uintptr_t)radiance & (half ? 7 : 15)) == 0, "%s: %s must be %d-byte aligned", who,
               aux || half ? "radiance" : "network_outputs", half ? 8 : 16);
  const bool pairs = K % 2 == 0 && (half ? ((uintptr_t)radiance & 15) == 0 : ((uintptr_t)ray_hit & 7) == 0);
  const float4* rad = static_cast<const float4*>(radiance);
  hipStream_t s = rtxn::as_stream(stream);
  const dim3 block(256), grid((batch_size + 3) / 4), pgrid((batch_size + 4 * kRaysPerWave - 1) / (4 * kRaysPerWave));
  auto launch = [&](auto mode_c, auto compact_c) {
    constexpr int MODE = decltype(mode_c)::value;
    constexpr bool COMPACT = decltype(compact_c)::value;
    if (aux) {
      if (pairs) volrender_aux_pair_kernel<MODE, COMPACT><<<pgrid, block, 0, s>>>(rad, num_hits, indices, ray_hit, batch_size, K, pixels, *aux);
      else volrender_aux_kernel<MODE, COMPACT><<<grid, block, 0, s>>>(rad, num_hits, indices, ray_hit, batch_size, K, pixels, *aux);
    } else {
      if (pairs) volrender_fwd_pair_kernel<MODE, COMPACT><<<pgrid, block, 0, s>>>(rad, num_hits, indices, ray_hit, batch_size, K, pixels);
      else volrender_fwd_kernel<MODE, COMPACT><<<grid, block, 0, s>>>(rad, num_hits, indices, ray_hit, batch_size, K, pixels);
    }
  };
  using compat = std::integral_constant<int, RTXN_VR_COMPAT>;
  using nerf = std::integral_constant<int, RTXN_VR_NERF>;
  if (half) {
    if (mode == RTXN_VR_COMPAT) launch(compat{}, std::true_type{});
    else launch(nerf{}, std::true_type{});
  } else {
    if (mode == RTXN_VR_COMPAT) launch(compat{}, std::false_type{});
    else launch(nerf{}, std::false_type{});
  }
  RTXN_LAUNCH_CHECK(what);
  return RTXN_OK;
}

}  // namespace

extern "C" int rtxn_volrender_fwd(const float* network_inputs, const float* network_outputs, const int* num_hits,
                                  const int* indices, const float* ray_hit, int batch_size,
                                  int num_samples_per_hit, float* pixels, int mode, rtxn_stream_t stream) {
  (void)network_inputs;  // unused by the reference as well (vol_render.cu:19-73)
  RTXN_REQUIRE(batch_size >= 0, "rtxn_volrender_fwd: batch_size = %d < 0", batch_size);
  RTXN_REQUIRE(num_samples_per_hit > 0, "rtxn_volrender_fwd: num_samples_per_hit = %d", num_samples_per_hit);
  RTXN_REQUIRE(mode == RTXN_VR_COMPAT || mode == RTXN_VR_NERF, "rtxn_volrender_fwd: unknown mode %d", mode);
  RTXN_DEVICE_OR_FAIL();
  if (batch_size == 0) return RTXN_OK;
  RTXN_REQUIRE(network_outputs && num_hits && indices && ray_hit && pixels, "rtxn_volrender_fwd: NULL buffer");
  return launch_fwd("rtxn_volrender_fwd", "volrender_fwd_kernel", network_outputs, false, mode, ray_hit, num_hits, indices, batch_size,
                    num_samples_per_hit, pixels, nullptr, stream);
}

extern "C" int rtxn_volrender_fwd_compact(const void* radiance_half4, const int* num_hits, const int* indices, int batch_size,
                                          int num_samples_per_hit, float* pixels, rtxn_stream_t stream) {
  RTXN_REQUIRE(batch_size >= 0, "rtxn_volrender_fwd_compact: batch_size = %d < 0", batch_size);
  RTXN_REQUIRE(num_samples_per_hit > 0, "rtxn_volrender_fwd_compact: num_samples_per_hit = %d", num_samples_per_hit);
  RTXN_DEVICE_OR_FAIL();
  if (batch_size == 0) return RTXN_OK;
  RTXN_REQUIRE(radiance_half4 && num_hits && indices && pixels, "rtxn_volrender_fwd_compact: NULL buffer");
  return launch_fwd("rtxn_volrender_fwd_compact", "volrender_fwd_kernel<compact>", radiance_half4, true, RTXN_VR_COMPAT, nullptr, num_hits,
                    indices, batch_size, num_samples_per_hit, pixels, nullptr, stream);
}

extern "C" int rtxn_volrender_fwd_compact_nerf(const void* radiance_half4, const float* segment_step, const int* num_hits,
                                               const int* indices, int batch_size, int num_samples_per_hit, float* pixels,
                                               rtxn_stream_t stream) {
  RTXN_REQUIRE(batch_size >= 0, "rtxn_volrender_fwd_compact_nerf: batch_size = %d < 0", batch_size);
  RTXN_REQUIRE(num_samples_per_hit > 0, "rtxn_volrender_fwd_compact_nerf: num_samples_per_hit = %d", num_samples_per_hit);
  RTXN_DEVICE_OR_FAIL();
  if (batch_size == 0) return RTXN_OK;
  RTXN_REQUIRE(radiance_half4 && segment_step && num_hits && indices && pixels, "rtxn_volrender_fwd_compact_nerf: NULL buffer");
  return launch_fwd("rtxn_volrender_fwd_compact_nerf", "volrender_fwd_kernel<compact, nerf>", radiance_half4, true, RTXN_VR_NERF,
                    segment_step, num_hits, indices, batch_size, num_samples_per_hit, pixels, nullptr, stream);
}

extern "C" int rtxn_volrender_bwd(const float* loss_values, const void* loss_gradients,
                                  const float* sampled_points_radiance, const float* t_hit, const int* num_hits,
                                  const int* indices, int batch_size, int num_samples_per_hit,
                                  void* radiance_gradients, int mode, rtxn_stream_t stream) {
  (void)loss_values;  // unused by the reference as well (vol_render.cu:75-143)
  RTXN_REQUIRE(batch_size >= 0, "rtxn_volrender_bwd: batch_size = %d < 0", batch_size);
  RTXN_REQUIRE(num_samples_per_hit > 0, "rtxn_volrender_bwd: num_samples_per_hit = %d", num_samples_per_hit);
  RTXN_REQUIRE(mode == RTXN_VR_COMPAT || mode == RTXN_VR_NERF, "rtxn_volrender_bwd: unknown mode %d", mode);
  RTXN_DEVICE_OR_FAIL();
  if (batch_size == 0) return RTXN_OK;
  RTXN_REQUIRE(loss_gradients && sampled_points_radiance && t_hit && num_hits && indices && radiance_gradients,
               "rtxn_volrender_bwd: NULL buffer");
  RTXN_REQUIRE(((uintptr_t)sampled_points_radiance & 15) == 0 && ((uintptr_t)radiance_gradients & 7) == 0,
               "rtxn_volrender_bwd: radiance must be 16-byte and gradients 8-byte aligned");
  hipStream_t s = rtxn::as_stream(stream);
  dim3 grid((batch_size + 3) / 4), block(256);
  const float4* rad = reinterpret_cast<const float4*>(sampled_points_radiance);
  const __half* lg = static_cast<const __half*>(loss_gradients);
  half4* out = static_cast<half4*>(radiance_gradients);
  if (mode == RTXN_VR_COMPAT)
    volrender_bwd_compat_kernel<<<grid, block, 0, s>>>(lg, rad, t_hit, num_hits, indices, batch_size,
                                                       num_samples_per_hit, out);
  else if (num_samples_per_hit % 2 == 0 && ((uintptr_t)t_hit & 7) == 0 && ((uintptr_t)radiance_gradients & 15) == 0)
    // the training compositor with the pixel gradients given instead of formed from a target: 512 samples per step, two per lane
    volrender_l2_fused_multi_kernel<4><<<grid, block, 0, s>>>(rad, t_hit, num_hits, indices, batch_size, num_samples_per_hit, nullptr, 0.0f,
                                                              nullptr, const_cast<__half*>(lg), nullptr, out);
  else
    volrender_bwd_nerf_kernel<<<grid, block, 0, s>>>(lg, rad, t_hit, num_hits, indices, batch_size,
                                                     num_samples_per_hit, out);
  RTXN_LAUNCH_CHECK("volrender_bwd_kernel");
  return RTXN_OK;
}

// rtxn_volrender_l2_train (bg == NULL: the plain kernels) and rtxn_volrender_l2_train_ex over an active background, behind
// rtxn::composite_train (composite_train.hip), which has checked the structs and names the entry point
int rtxn::l2_train(const char* who, const rtxn::CompositeArgs& c, const rtxn_train_background* active_bg, rtxn_stream_t stream) {
  const int batch_size = c.batch_size, K = c.num_samples_per_hit;
  RTXN_REQUIRE(batch_size >= 0, "%s: batch_size = %d < 0", who, batch_size);
  RTXN_REQUIRE(K > 0, "%s: num_samples_per_hit = %d", who, K);
  RTXN_DEVICE_OR_FAIL();
  hipStream_t s = rtxn::as_stream(stream);
  // deterministic mode: the kernels get no loss pointer (their sum is float atomics, per block or per ray); loss.hip sums behind them
  const bool det_loss = c.loss_sum && batch_size > 0 && rtxn::deterministic_mode();
  if (c.loss_sum && !det_loss) RTXN_HIP(rtxn::zero_words(c.loss_sum, 1, s));
  if (batch_size == 0) return RTXN_OK;
  RTXN_REQUIRE(c.network_outputs && c.ray_hit && c.num_hits && c.indices && c.target && c.pixels && c.radiance_gradients, "%s: NULL buffer", who);
  float* const loss_sum = det_loss ? nullptr : c.loss_sum;
  RTXN_REQUIRE(((uintptr_t)c.network_outputs & 15) == 0 && ((uintptr_t)c.radiance_gradients & 7) == 0,
               "%s: radiance must be 16-byte and gradients 8-byte aligned", who);
  // 512 samples per step, two per lane: an even K, 8-byte-aligned step lengths and 16-byte-aligned gradients
  const bool pairs = K % 2 == 0 && ((uintptr_t)c.ray_hit & 7) == 0 && ((uintptr_t)c.radiance_gradients & 15) == 0;
  const dim3 grid((batch_size + 3) / 4), block(256);
  const float4* rad = reinterpret_cast<const float4*>(c.network_outputs);
  __half* lg = static_cast<__half*>(c.loss_gradients_half);
  half4* out = static_cast<half4*>(c.radiance_gradients);
  const BgArgs bg = make_bg_args(active_bg);
  if (active_bg) {
    if (pairs) volrender_l2_bg_multi_kernel<4><<<grid, block, 0, s>>>(rad, c.ray_hit, c.num_hits, c.indices, batch_size, K, c.target, c.loss_scale, c.pixels, lg, loss_sum, out, bg);
    else volrender_l2_bg_kernel<<<grid, block, 0, s>>>(rad, c.ray_hit, c.num_hits, c.indices, batch_size, K, c.target, c.loss_scale, c.pixels, lg, loss_sum, out, bg);
    RTXN_LAUNCH_CHECK("volrender_l2_bg_kernel");
  } else {
    if (pairs) volrender_l2_fused_multi_kernel<4><<<grid, block, 0, s>>>(rad, c.ray_hit, c.num_hits, c.indices, batch_size, K, c.target, c.loss_scale, c.pixels, lg, loss_sum, out);
    else volrender_l2_fused_kernel<<<grid, block, 0, s>>>(rad, c.ray_hit, c.num_hits, c.indices, batch_size, K, c.target, c.loss_scale, c.pixels, lg, loss_sum, out);
    RTXN_LAUNCH_CHECK("volrender_l2_fused_kernel");
  }
  if (det_loss)
    return rtxn::l2_loss_fixed_order(c.pixels, c.target, batch_size, bg.mode, active_bg ? bg.color : nullptr, bg.seed, bg.step, bg.target_channels,
                                     c.loss_sum, s);
  return RTXN_OK;
}

extern "C" int rtxn_volrender_l2_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                                       int batch_size, int num_samples_per_hit, const float* target, float loss_scale,
                                       float* pixels, void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                                       rtxn_stream_t stream) {
  return rtxn::composite_train("rtxn_volrender_l2_train", {network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target,
                               loss_scale, pixels, loss_gradients_half, loss_sum, radiance_gradients}, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int rtxn_volrender_l2_train_ex(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                                          int batch_size, int num_samples_per_hit, const float* target, float loss_scale,
                                          float* pixels, void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                                          const rtxn_train_background* bg, rtxn_stream_t stream) {
  return rtxn::composite_train("rtxn_volrender_l2_train_ex", {network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target,
                               loss_scale, pixels, loss_gradients_half, loss_sum, radiance_gradients}, bg, nullptr, nullptr, nullptr, stream);
}

extern "C" int rtxn_volrender_fwd_aux(const void* radiance, int radiance_layout, const float* ray_hit, const int* num_hits,
                                      const int* indices, const float* t_start, const float* t_end, int batch_size,
                                      int num_samples_per_hit, int vr_mode, int sample_type, const float* background,
                                      float* pixels, float* depth, float* opacity, rtxn_stream_t stream) {
  RTXN_REQUIRE(batch_size >= 0, "rtxn_volrender_fwd_aux: batch_size = %d < 0", batch_size);
  RTXN_REQUIRE(num_samples_per_hit > 0, "rtxn_volrender_fwd_aux: num_samples_per_hit = %d", num_samples_per_hit);
  RTXN_REQUIRE(vr_mode == RTXN_VR_COMPAT || vr_mode == RTXN_VR_NERF, "rtxn_volrender_fwd_aux: unknown mode %d", vr_mode);
  RTXN_REQUIRE(radiance_layout == RTXN_RADIANCE_FLOAT4 || radiance_layout == RTXN_RADIANCE_HALF4,
               "rtxn_volrender_fwd_aux: unknown radiance layout %d", radiance_layout);
  RTXN_REQUIRE(sample_type == RTXN_SAMPLING_REGULAR || sample_type == RTXN_SAMPLING_MIDPOINT_WORLD,
               "rtxn_volrender_fwd_aux: sample_type %d (the deterministic modes only: REGULAR, MIDPOINT_WORLD)", sample_type);
  RTXN_REQUIRE(!depth || (t_start && t_end), "rtxn_volrender_fwd_aux: depth needs t_start and t_end");
  RTXN_DEVICE_OR_FAIL();
  if (batch_size == 0) return RTXN_OK;
  const bool half = radiance_layout == RTXN_RADIANCE_HALF4;
  RTXN_REQUIRE(radiance && num_hits && indices && pixels && (ray_hit || (half && vr_mode == RTXN_VR_COMPAT)),
               "rtxn_volrender_fwd_aux: NULL buffer");
  AuxArgs aux;
  aux.t_start = t_start;
  aux.t_end = t_end;
  aux.u0 = sample_type == RTXN_SAMPLING_MIDPOINT_WORLD ? 0.5f : 0.0f;
  for (int c = 0; c < 3; ++c) aux.bg[c] = background ? background[c] : 0.0f;
  aux.depth = depth;
  aux.opacity = opacity;
  return launch_fwd("rtxn_volrender_fwd_aux", "volrender_aux_kernel", radiance, half, vr_mode, ray_hit, num_hits, indices, batch_size,
                    num_samples_per_hit, pixels, &aux, stream);
}
