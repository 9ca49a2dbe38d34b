// The training compositor for the losses of rtxn_train_loss and the distortion regulariser of rtxn_train_regularizer
// (include/rtxn.h): rtxn_volrender_l2_train_ex's two sweeps with the per-ray step between them -- pixel,
// loss value, fp16 loss gradient -- evaluated by loss_internal.h's loss_term instead of the hard-wired L2, plus the alpha term
// lambda (A - alpha)^2, whose gradient g_A enters the second sweep as one more constant beside the background's dot product:
//   dL/dw_k = g.c_k - g.b + g_A,   S = g.(sum w c) - (g.b) A + g_A A.
// With REG the distortion term is added, per ray over its samples in storage order (ascending, disjoint t):
//   L_r = 2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 delta_i,      W_<i = sum_{j<i} w_j,  M_<i = sum_{j<i} w_j m_j,
//   q_i = dL_r/dw_i = 2 [m_i (2 W_<i + w_i - A) - (2 M_<i + w_i m_i - B)] + (2/3) w_i delta_i,     A = sum w,  B = sum w m,
// m_i the midpoint and delta_i the width of the sample's sub-interval, both from the segment's t_start / t_end, read beside the
// radiance (the step lengths the compositor reads carry rtxn_train_batch.t_scale, a factor on sigma and not a distance).
// Sweep 1 accumulates L_r beside the colour sums from the running prefixes of w and w m (two more scans per step); sweep 2
// re-forms the prefixes and adds k q_i, k = loss_scale lambda_d / n_rays in fp32, to gc:
//   dL/dw_i = g.c_i - g.b + g_A + k q_i,   S = g.(sum w c) - (g.b) A + g_A A + 2 k L_r     (sum_i w_i q_i = 2 L_r).
// Two schedules, each ONE kernel template on REG: what the regulariser adds sits under `if constexpr (REG)`, so REG = false is
// the loss compositor by construction.  The kernel itself is the template, not a wrapper round an inlined body, and the
// per-ray sample index is long without the regulariser and int with it (which divides by K): DESIGN 5.12 has the
// measurements behind both.  The volrender_l2_* kernels (volrender.hip) stay copies of these schedules: their machine code is
// pinned by tests/test_compositor_isa.py.  Loss kind, parameter, lambda and the background flag are wave-uniform values of an
// argument struct; the loss is evaluated once per ray on three channels, so the kernels are not instantiated per kind.
// DEV (rtxn_volrender_scaled_train): the loss scale is a word of device memory (rtxn_loss_scaler_state::scale) instead
// of an argument -- the argument's type and the two reads through scale_value() are all that differs, so DEV = false is the
// by-value kernel byte for byte (profiles/r14/compositor_scaled_ab.txt).
// DEPTH (rtxn_train_depth), which implies REG: the ray's expected depth D_r = B = sum w m, which the REG kernels
// carry already, is fitted to a per-ray target z_r: with e_r = D_r - z_r on rays with a target, the share gains
// (lambda_z / n_rays) l(e_r), and sweep 2 one more addend, in fp32 as k q_i is:
//   dL/dw_i = ... + g_D m_i,   S = ... + g_D D_r,   g_D = k_z l'(e_r),  k_z = loss_scale lambda_z / n_rays   (D_r is of degree 1 in w).
// Everything it adds sits under `if constexpr (DEPTH)`; its arguments ride behind RegArgs in the last kernel argument
// (RegDepthArgs), so the other instantiations keep their argument block and their machine code
// (profiles/r25/compositor_fingerprints*.txt).
#include <cmath>
#include <type_traits>

#include "background_internal.h"
#include "common.h"
#include "depth_internal.h"
#include "loss_internal.h"
#include "reg_internal.h"
#include "wave_scan_internal.h"

namespace {

// a ray's sample count and loop index
template <bool REG>
using sample_index = std::conditional_t<REG, int, long>;

// The loss scale of a launch: the by-value argument, or (DEV) the word rtxn_loss_scaler keeps in device memory.  The pointer is a
// kernel argument and the address is the same in every lane, so the read is one scalar load per wave, not a load per lane.
template <bool DEV>
using scale_arg = std::conditional_t<DEV, const float*, float>;
__device__ __forceinline__ float scale_value(float s) { return s; }
__device__ __forceinline__ float scale_value(const float* s) { return *s; }

// What a ray's wave does between the sweeps: pixel, loss gradient (fp16, stored and handed on in that form), the ray's share of
// the loss -- with REG the regulariser's included -- and the per-ray outputs; returns the share.  Every value is wave-uniform;
// lane 0 stores.
// DEPTH (rtxn_train_depth): the ray's depth target is read, l(e_r) joins the share and g_D = kz l'(e_r) is handed to
// sweep 2 in fp32; kz and gD are not touched otherwise.
struct RayGrad {
  float g0, g1, g2, gA;
};
template <bool REG, bool DEPTH>
__device__ __forceinline__ float ray_step(const BgArgs& bga, const LossArgs& la, const reg_args<DEPTH>& ra, const float* __restrict__ target, int ray,
                                          int batch_size, int lane, float loss_scale, float ar, float ag, float ab, float aw, float L, float B,
                                          float* __restrict__ pixels, __half* __restrict__ loss_gradients, float (&bg)[3], RayGrad& g, float kz,
                                          float& gD) {
  const float inv_n = 1.0f / (float)(3L * batch_size), inv_rays = 1.0f / (float)batch_size;
  float tg[3];
  ray_background(bga, target, ray, bg, tg);
  float p[3] = {ar, ag, ab};
  if (la.has_background) {
    const float rest = 1.0f - aw;
    p[0] = fmaf(rest, bg[0], ar);
    p[1] = fmaf(rest, bg[1], ag);
    p[2] = fmaf(rest, bg[2], ab);
  }
  const float alpha = bga.target_channels == 4 ? target[4 * (long)ray + 3] : 0.0f;
  float dl[3], dA;
  float value = ray_loss_term(la, p, tg, aw, alpha, inv_n, inv_rays, dl, dA);
  if constexpr (REG) {
    if (ra.weight > 0.0f) value += reg_loss_share(ra.weight, L, inv_rays);
  }
  float lz = 0.0f;
  if constexpr (DEPTH) {
    float dlz;
    lz = depth_term(ra.z, B, ra.z.target[ray], dlz);
    gD = kz * dlz;
    if (ra.z.weight > 0.0f) value += depth_loss_share(ra.z.weight, lz, inv_rays);
  }
  const __half h0 = loss_grad_half(loss_scale, dl[0], inv_n), h1 = loss_grad_half(loss_scale, dl[1], inv_n),
               h2 = loss_grad_half(loss_scale, dl[2], inv_n);
  g.g0 = __half2float(h0);
  g.g1 = __half2float(h1);
  g.g2 = __half2float(h2);
  g.gA = la.opacity_weight > 0.0f ? __half2float(opacity_grad_half(loss_scale, la.opacity_weight, dA, inv_rays)) : 0.0f;
  if (lane == 0) {
    pixels[3 * (long)ray] = p[0];
    pixels[3 * (long)ray + 1] = p[1];
    pixels[3 * (long)ray + 2] = p[2];
    if (loss_gradients) {
      loss_gradients[3 * (long)ray] = h0;
      loss_gradients[3 * (long)ray + 1] = h1;
      loss_gradients[3 * (long)ray + 2] = h2;
    }
    if (la.opacity) la.opacity[ray] = aw;
    if constexpr (REG) {
      if (ra.distortion) ra.distortion[ray] = L;
      if (ra.depth) ra.depth[ray] = B;
    }
    if constexpr (DEPTH) {
      if (ra.z.depth) ra.z.depth[ray] = B;
      if (ra.z.depth_loss) ra.z.depth_loss[ray] = lz;
    }
  }
  return value;
}

// one ray per wave, 64 samples per step: the form for odd K or misaligned buffers (volrender_l2_bg_kernel's schedule).
// Both instantiations of both kernels are, byte for byte, the machine code of the four kernels they replace
// (profiles/r12/compositor_merge_ab.txt), and that holds only for this arrangement of the local declarations: the compiler
// promotes locals to registers in an order that follows where and how each is declared, and the later passes follow that
// order -- a local that an instantiation never uses included.  Hence, in sweep 2, m and dw stand in a statement of their own
// ahead of d, wi, mi and q are declared outside the loop and assigned under `if constexpr` (through wi_, mi_), gc is updated
// in place; in the pair kernel w0, w1, q0, q1 are declared without a value and the loss instantiation forms Ti (1 - ex)
// inside the product with gc.  Re-run the comparison after moving a declaration in either kernel.
template <bool REG, bool DEV, bool DEPTH = false>
__global__ __launch_bounds__(256) void composite_train_kernel(const float4* __restrict__ radiance, const float* __restrict__ step_len,
                                                              const int* __restrict__ num_hits, const int* __restrict__ indices,
                                                              int batch_size, int K, const float* __restrict__ target,
                                                              scale_arg<DEV> loss_scale,
                                                              float* __restrict__ pixels, __half* __restrict__ loss_gradients,
                                                              float* __restrict__ loss_sum, half4* __restrict__ grads, BgArgs bga, LossArgs la,
                                                              reg_args<DEPTH> ra) {
  static_assert(REG || !DEPTH, "the depth term needs the regulariser's midpoints and its sum w m");
  using idx_t = sample_index<REG>;
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= batch_size) return;
  const long seg0 = (long)indices[ray];
  const long base = seg0 * K;
  const idx_t n = (idx_t)num_hits[ray] * K;
  const float rK = 1.0f / (float)K;
  auto interval = [&](int i, float& m, float& dw) {
    const int j = i / K;
    const float ts = ra.t_start[seg0 + j], te = ra.t_end[seg0 + j];
    m = reg_midpoint(i - j * K, rK, ts, te);
    dw = reg_width(rK, ts, te);
  };
  // sweep 1: colour and opacity sums; REG: sum w m and the two sums of L_r
  float T_carry = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f;
  float W_carry = 0.0f, M_carry = 0.0f, lp = 0.0f, ls = 0.0f;
  for (idx_t s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float d = 0.0f, m = 0.0f, dw = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      d = step_len[base + s0 + lane];
      if constexpr (REG) interval(s0 + lane, m, dw);
    }
    const float x = d * c.w;
    const float incl = wave_incl_scan_f(x);
    const float w = act ? expf(-(T_carry + incl - x)) * (1.0f - expf(-x)) : 0.0f;
    ar = fmaf(w, c.x, ar);
    ag = fmaf(w, c.y, ag);
    ab = fmaf(w, c.z, ab);
    aw += w;
    T_carry += lane63(incl);
    if constexpr (REG) {
      const float wm = w * m;
      const float wi = wave_incl_scan_f(w), mi = wave_incl_scan_f(wm);
      const float Wlt = W_carry + (wi - w), Mlt = M_carry + (mi - wm);
      lp += w * (m * Wlt - Mlt);
      ls += (w * w) * dw;
      W_carry += lane63(wi);
      M_carry += lane63(mi);
    }
  }
  ar = wave_sum(ar);
  ag = wave_sum(ag);
  ab = wave_sum(ab);
  aw = wave_sum(aw);
  const float L = REG ? reg_ray_value(wave_sum(lp), wave_sum(ls)) : 0.0f;
  const float Wt = W_carry, Bt = M_carry;             // REG: A and B as the prefixes of sweep 2 will sum them
  float bg[3];
  RayGrad g;
  float gD = 0.0f;                                    // DEPTH: k_z l'(e_r), 0 for a ray without a target
  float kz = 0.0f;
  if constexpr (DEPTH) kz = depth_k<DEV>(ra.z, scale_value(loss_scale), batch_size);
  const float value = ray_step<REG, DEPTH>(bga, la, ra, target, ray, batch_size, lane, scale_value(loss_scale), ar, ag, ab, aw, L, Bt, pixels,
                                           loss_gradients, bg, g, kz, gD);
  if (lane == 0 && loss_sum) atomicAdd(loss_sum, value);
  const float g0 = g.g0, g1 = g.g1, g2 = g.g2;
  const float gbg = g0 * bg[0] + g1 * bg[1] + g2 * bg[2];
  const float kq = reg_k<DEV>(ra, scale_value(loss_scale), batch_size);
  const float S0 = ((g0 * ar + g1 * ag + g2 * ab) - gbg * aw) + g.gA * aw;     // = sum_k w_k (g . (c_k - bg) + g_A)
  float S = REG ? S0 + 2.0f * kq * L : S0;
  if constexpr (DEPTH) S += gD * Bt;                  // a ray without a target: gD = 0, every value is that of the call without the term
  // sweep 2: per-sample gradients
  T_carry = 0.0f;
  if constexpr (REG) W_carry = M_carry = 0.0f;
  float P_carry = 0.0f;
  float wi, mi, q;                                    // REG: a step's two scans and q_i
  for (idx_t s0 = 0; s0 < n; s0 += 64) {
    const bool act = s0 + lane < n;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float m = 0.0f, dw = 0.0f;                        // REG
    float d = 0.0f;
    if (act) {
      c = radiance[base + s0 + lane];
      d = step_len[base + s0 + lane];
      if constexpr (REG) interval(s0 + lane, m, dw);
    }
    const float x = d * c.w;
    const float incl = wave_incl_scan_f(x);
    const float Ti = expf(-(T_carry + incl - x));
    const float ex = expf(-x);
    const float a = 1.0f - ex;
    if constexpr (REG) {
      const float w = act ? Ti * a : 0.0f, wm = w * m;
      const float wi_ = wave_incl_scan_f(w), mi_ = wave_incl_scan_f(wm);
      wi = wi_;                                       // kept for the carries at the end of the step
      mi = mi_;
      const float Wlt = W_carry + (wi - w), Mlt = M_carry + (mi - wm);
      q = 2.0f * (m * ((2.0f * Wlt + w) - Wt) - ((2.0f * Mlt + wm) - Bt)) + (2.0f / 3.0f) * (w * dw);
    }
    float gc = ((g0 * c.x + g1 * c.y + g2 * c.z) - gbg) + g.gA;
    if constexpr (REG) gc += kq * q;
    if constexpr (DEPTH) gc += gD * m;
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
    if constexpr (REG) {
      W_carry += lane63(wi);
      M_carry += lane63(mi);
    }
  }
}

// U blocks of 128 samples per step, two per lane (volrender_l2_bg_multi_kernel's schedule and arithmetic): even K, 8-byte
// aligned step lengths, 16-byte aligned gradients.  The loss is reduced per block and added once per block at the very end.
// REG: a pair never straddles two segments (K even): one t_start / t_end pair per lane and block, turned into the pair's two
// midpoints and their common width as it is loaded.
template <bool REG, int U, bool DEV, bool DEPTH = false>
__global__ __launch_bounds__(256) void composite_train_multi_kernel(const float4* __restrict__ radiance, const float* __restrict__ step_len,
                                                                    const int* __restrict__ num_hits, const int* __restrict__ indices,
                                                                    int batch_size, int K, const float* __restrict__ target,
                                                                    scale_arg<DEV> loss_scale, float* __restrict__ pixels,
                                                                    __half* __restrict__ loss_gradients, float* __restrict__ loss_sum,
                                                                    half4* __restrict__ grads, BgArgs bga, LossArgs la,
                                                                    reg_args<DEPTH> ra) {
  static_assert(REG || !DEPTH, "the depth term needs the regulariser's midpoints and its sum w m");
  using idx_t = sample_index<REG>;
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ray = blockIdx.x * 4 + wave;
  float loss_part = 0.0f;
  if (ray < batch_size) {
    const long seg0 = (long)indices[ray];
    const long base = seg0 * K;
    const idx_t n = (idx_t)num_hits[ray] * K;          // even
    const float rK = 1.0f / (float)K;
    const int kmask = (K & (K - 1)) == 0 ? K - 1 : 0;
    const int kshift = kmask ? __builtin_ctz((unsigned)K) : 0;
    constexpr idx_t STEP = 128 * U;
    struct Pair { float4 c0, c1; float d0, d1, m0, m1, dw; };      // m0, m1, dw: REG only
    auto load = [&](idx_t s0, Pair (&p)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const idx_t i0 = s0 + 128 * u + 2 * lane;
        p[u].c0 = p[u].c1 = make_float4(0.f, 0.f, 0.f, 0.f);
        p[u].d0 = p[u].d1 = p[u].m0 = p[u].m1 = p[u].dw = 0.0f;
        if (i0 < n) {
          p[u].c0 = radiance[base + i0];
          p[u].c1 = radiance[base + i0 + 1];
          const float2 dd = *reinterpret_cast<const float2*>(step_len + base + i0);
          p[u].d0 = dd.x;
          p[u].d1 = dd.y;
          if constexpr (REG) {
            const int j = kmask ? i0 >> kshift : i0 / K;
            const int k0 = kmask ? (i0 & kmask) : i0 - j * K;
            const float ts = ra.t_start[seg0 + j], te = ra.t_end[seg0 + j];
            p[u].m0 = reg_midpoint(k0, rK, ts, te);
            p[u].m1 = reg_midpoint(k0 + 1, rK, ts, te);
            p[u].dw = reg_width(rK, ts, te);
          }
        }
      }
    };
    // sweep 1: colour and opacity sums; REG: sum w m and the two sums of L_r
    float T_carry = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f;
    float W_carry = 0.0f, M_carry = 0.0f, lp = 0.0f, ls = 0.0f;
    Pair cur[U], nxt[U];
    if (n > 0) load(0, cur);
    for (idx_t s0 = 0; s0 < n; s0 += STEP) {
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
        if constexpr (REG) {
          const float wm0 = w0 * cur[u].m0, wm1 = w1 * cur[u].m1;
          const float pw = w0 + w1, pm = wm0 + wm1;
          const float wi = wave_incl_scan_f(pw), mi = wave_incl_scan_f(pm);
          const float Wlt0 = W_carry + (wi - pw), Mlt0 = M_carry + (mi - pm);
          lp += w0 * (cur[u].m0 * Wlt0 - Mlt0);
          lp += w1 * (cur[u].m1 * (Wlt0 + w0) - (Mlt0 + wm0));
          ls += ((w0 * w0) + (w1 * w1)) * cur[u].dw;
          W_carry += lane63(wi);
          M_carry += lane63(mi);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
    ar = wave_sum(ar);
    ag = wave_sum(ag);
    ab = wave_sum(ab);
    aw = wave_sum(aw);
    const float L = REG ? reg_ray_value(wave_sum(lp), wave_sum(ls)) : 0.0f;
    const float Wt = W_carry, Bt = M_carry;           // REG: A and B as the prefixes of sweep 2 will sum them
    float bg[3];
    RayGrad g;
    float gD = 0.0f;                                  // DEPTH: k_z l'(e_r), 0 for a ray without a target
    float kz = 0.0f;
    if constexpr (DEPTH) kz = depth_k<DEV>(ra.z, scale_value(loss_scale), batch_size);
    loss_part = ray_step<REG, DEPTH>(bga, la, ra, target, ray, batch_size, lane, scale_value(loss_scale), ar, ag, ab, aw, L, Bt, pixels,
                                     loss_gradients, bg, g, kz, gD);
    const float g0 = g.g0, g1 = g.g1, g2 = g.g2;
    const float gbg = g0 * bg[0] + g1 * bg[1] + g2 * bg[2];
    const float kq = reg_k<DEV>(ra, scale_value(loss_scale), batch_size);
    const float S0 = ((g0 * ar + g1 * ag + g2 * ab) - gbg * aw) + g.gA * aw;     // = sum_k w_k (g . (c_k - bg) + g_A)
    float S = REG ? S0 + 2.0f * kq * L : S0;
    if constexpr (DEPTH) S += gD * Bt;                // a ray without a target: gD = 0, every value is that of the call without the term
    // sweep 2: per-sample gradients (the radiance is re-read: cache hits)
    T_carry = 0.0f;
    if constexpr (REG) W_carry = M_carry = 0.0f;
    float P_carry = 0.0f;
    if (n > 0) load(0, cur);
    for (idx_t s0 = 0; s0 < n; s0 += STEP) {
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
        // inactive lanes: w = Ti (1 - ex) = 0 (x = 0) and m = 0, so the constants of their zero colour add nothing to any prefix
        float w0, w1, q0, q1;                            // REG
        if constexpr (REG) {
          w0 = Ti0[u] * (1.0f - ex0[u]);
          w1 = Ti1[u] * (1.0f - ex1[u]);
          const float m0 = cur[u].m0, m1 = cur[u].m1;
          const float wm0 = w0 * m0, wm1 = w1 * m1;
          const float pw = w0 + w1, pm = wm0 + wm1;
          const float wi = wave_incl_scan_f(pw), mi = wave_incl_scan_f(pm);
          const float Wlt0 = W_carry + (wi - pw), Mlt0 = M_carry + (mi - pm);
          const float Wlt1 = Wlt0 + w0, Mlt1 = Mlt0 + wm0;
          W_carry += lane63(wi);
          M_carry += lane63(mi);
          q0 = 2.0f * (m0 * ((2.0f * Wlt0 + w0) - Wt) - ((2.0f * Mlt0 + wm0) - Bt)) + (2.0f / 3.0f) * (w0 * cur[u].dw);
          q1 = 2.0f * (m1 * ((2.0f * Wlt1 + w1) - Wt) - ((2.0f * Mlt1 + wm1) - Bt)) + (2.0f / 3.0f) * (w1 * cur[u].dw);
        }
        gc0[u] = ((g0 * cur[u].c0.x + g1 * cur[u].c0.y + g2 * cur[u].c0.z) - gbg) + g.gA;
        if constexpr (REG) gc0[u] += kq * q0;
        gc1[u] = ((g0 * cur[u].c1.x + g1 * cur[u].c1.y + g2 * cur[u].c1.z) - gbg) + g.gA;
        if constexpr (REG) gc1[u] += kq * q1;
        if constexpr (DEPTH) {
          gc0[u] += gD * cur[u].m0;
          gc1[u] += gD * cur[u].m1;
        }
        const float wgc0 = (REG ? w0 : Ti0[u] * (1.0f - ex0[u])) * gc0[u];
        wgc1[u] = (REG ? w1 : Ti1[u] * (1.0f - ex1[u])) * gc1[u];
        pin[u] = wave_incl_scan_f(wgc0 + wgc1[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const idx_t i0 = s0 + 128 * u + 2 * lane;
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

// The one RTXN_VR_NERF training compositor (common.h): the five rtxn_volrender_*_train entry points and rtxn_train_gradients.
int rtxn::composite_train(const char* who, const rtxn::CompositeArgs& c, const rtxn_train_background* bg, const rtxn_train_loss* loss,
                          const rtxn_train_regularizer* reg, const float* scale_dev, rtxn_stream_t stream, const rtxn_train_depth* depth) {
  bool bg_active = false, loss_active = false, reg_active = false, depth_active = false;
  int rc = rtxn::check_train_background(bg, RTXN_VR_NERF, who, &bg_active);
  if (rc != RTXN_OK) return rc;
  rc = rtxn::check_train_loss(loss, bg_active ? bg->target_channels : 3, RTXN_VR_NERF, who, &loss_active);
  if (rc != RTXN_OK) return rc;
  rc = rtxn::check_train_regularizer(reg, RTXN_VR_NERF, -1, who, &reg_active);
  if (rc != RTXN_OK) return rc;
  if (!bg_active) bg = nullptr;
  if (!loss_active) loss = nullptr;
  if (!reg_active) reg = nullptr;
  rc = rtxn::check_train_depth(depth, reg, nullptr, RTXN_VR_NERF, -1, who, &depth_active);
  if (rc != RTXN_OK) return rc;
  if (!depth_active) depth = nullptr;
  // An inactive struct runs exactly what the entry point without it runs, under that entry point's name.  With scale_dev nothing
  // falls through: plain L2 is one of loss_term's kinds.
  if (!scale_dev) {
    if (!reg && !loss && !depth) return rtxn::l2_train(bg ? "rtxn_volrender_l2_train_ex" : "rtxn_volrender_l2_train", c, bg, stream);
    who = depth ? "rtxn_volrender_depth_train" : reg ? "rtxn_volrender_reg_train" : "rtxn_volrender_loss_train";
  }
  const int batch_size = c.batch_size, num_samples_per_hit = c.num_samples_per_hit;
  RTXN_REQUIRE(batch_size >= 0, "%s: batch_size = %d < 0", who, batch_size);
  RTXN_REQUIRE(num_samples_per_hit > 0, "%s: num_samples_per_hit = %d", who, num_samples_per_hit);
  // deterministic mode: the kernels get no loss pointer (their sum is float atomics); loss.hip sums behind them
  const bool det_loss = c.loss_sum && batch_size > 0 && rtxn::deterministic_mode();
  RTXN_REQUIRE(!(det_loss && loss && loss->opacity_weight > 0.0f && !loss->opacity),
               "%s: loss->opacity is NULL: in deterministic mode the alpha term of the loss is summed from the opacities the compositor writes there",
               who);
  RTXN_REQUIRE(!(det_loss && reg && reg->distortion_weight > 0.0f && !reg->distortion),
               "%s: reg->distortion is NULL: in deterministic mode the distortion term of the loss is summed from the L_r the compositor writes there",
               who);
  RTXN_REQUIRE(!(det_loss && depth && depth->weight > 0.0f && !depth->depth),
               "%s: depth->depth is NULL: in deterministic mode the depth term of the loss is summed from the D_r the compositor writes there",
               who);
  RTXN_DEVICE_OR_FAIL();
  hipStream_t s = rtxn::as_stream(stream);
  if (c.loss_sum && !det_loss) RTXN_HIP(rtxn::zero_words(c.loss_sum, 1, s));
  if (batch_size == 0) return RTXN_OK;
  RTXN_REQUIRE(c.network_outputs && c.ray_hit && c.num_hits && c.indices && c.target && c.pixels && c.radiance_gradients, "%s: NULL buffer", who);
  RTXN_REQUIRE(((uintptr_t)c.network_outputs & 15) == 0 && ((uintptr_t)c.radiance_gradients & 7) == 0,
               "%s: radiance must be 16-byte and gradients 8-byte aligned", who);
  const BgArgs a = make_bg_args(bg);
  const LossArgs la = make_loss_args(loss, bg != nullptr);
  const RegArgs ra = make_reg_args(reg, c.loss_scale, batch_size);
  // 512 samples per step, two per lane: an even K, 8-byte-aligned step lengths and 16-byte-aligned gradients
  const bool pairs = num_samples_per_hit % 2 == 0 && ((uintptr_t)c.ray_hit & 7) == 0 && ((uintptr_t)c.radiance_gradients & 15) == 0;
  const dim3 grid((batch_size + 3) / 4), block(256);
  const float4* const rad = reinterpret_cast<const float4*>(c.network_outputs);
  __half* const lg = static_cast<__half*>(c.loss_gradients_half);
  float* const ls = det_loss ? nullptr : c.loss_sum;
  half4* const rg = static_cast<half4*>(c.radiance_gradients);
  if (depth) {
    // the depth term: the REG kernels with one more addend; without a regulariser of its own lambda_d = 0 over the depth struct's distances
    RegDepthArgs rz{};
    static_cast<RegArgs&>(rz) = ra;
    if (!reg) {
      rz.t_start = depth->t_start;
      rz.t_end = depth->t_end;
    }
    rz.z = make_depth_args(depth, c.loss_scale, batch_size);
    if (scale_dev) {
      auto* const kernel = pairs ? composite_train_multi_kernel<true, 4, true, true> : composite_train_kernel<true, true, true>;
      kernel<<<grid, block, 0, s>>>(rad, c.ray_hit, c.num_hits, c.indices, batch_size, num_samples_per_hit, c.target, scale_dev, c.pixels, lg, ls, rg, a, la, rz);
    } else {
      auto* const kernel = pairs ? composite_train_multi_kernel<true, 4, false, true> : composite_train_kernel<true, false, true>;
      kernel<<<grid, block, 0, s>>>(rad, c.ray_hit, c.num_hits, c.indices, batch_size, num_samples_per_hit, c.target, c.loss_scale, c.pixels, lg, ls, rg, a, la, rz);
    }
  } else if (scale_dev) {
    auto* const kernel = reg ? (pairs ? composite_train_multi_kernel<true, 4, true> : composite_train_kernel<true, true>)
                             : (pairs ? composite_train_multi_kernel<false, 4, true> : composite_train_kernel<false, true>);
    kernel<<<grid, block, 0, s>>>(rad, c.ray_hit, c.num_hits, c.indices, batch_size, num_samples_per_hit, c.target, scale_dev, c.pixels, lg, ls, rg, a, la, ra);
  } else {
    auto* const kernel = reg ? (pairs ? composite_train_multi_kernel<true, 4, false> : composite_train_kernel<true, false>)
                             : (pairs ? composite_train_multi_kernel<false, 4, false> : composite_train_kernel<false, false>);
    kernel<<<grid, block, 0, s>>>(rad, c.ray_hit, c.num_hits, c.indices, batch_size, num_samples_per_hit, c.target, c.loss_scale, c.pixels, lg, ls, rg, a, la, ra);
  }
  RTXN_LAUNCH_CHECK("composite_train_kernel");
  if (det_loss) return rtxn::loss_fixed_order(c.pixels, c.target, batch_size, bg, loss, reg, depth, c.loss_sum, s);
  return RTXN_OK;
}

int rtxn::check_train_loss(const rtxn_train_loss* loss, int target_channels, int vr_mode, const char* who, bool* active) {
  *active = false;
  if (!loss) return RTXN_OK;
  RTXN_REQUIRE(loss->kind == RTXN_LOSS_L2 || loss->kind == RTXN_LOSS_L1 || loss->kind == RTXN_LOSS_HUBER || loss->kind == RTXN_LOSS_RELATIVE_L2,
               "%s: loss->kind = %d: unknown loss kind (RTXN_LOSS_L2 | _L1 | _HUBER | _RELATIVE_L2)", who, loss->kind);
  if (loss->kind == RTXN_LOSS_HUBER)
    RTXN_REQUIRE(std::isfinite(loss->param) && loss->param > 0.0f, "%s: loss->param = %g: RTXN_LOSS_HUBER needs a finite delta > 0", who,
                 (double)loss->param);
  if (loss->kind == RTXN_LOSS_RELATIVE_L2)
    RTXN_REQUIRE(std::isfinite(loss->param) && loss->param > 0.0f, "%s: loss->param = %g: RTXN_LOSS_RELATIVE_L2 needs a finite epsilon > 0", who,
                 (double)loss->param);
  RTXN_REQUIRE(loss->opacity_weight >= 0.0f && std::isfinite(loss->opacity_weight), "%s: loss->opacity_weight = %g (finite, >= 0)", who,
               (double)loss->opacity_weight);
  if (vr_mode < 0) {
    RTXN_REQUIRE(loss->opacity_weight == 0.0f && !loss->opacity,
                 "%s: loss->opacity_weight / loss->opacity need a compositor (rtxn_volrender_loss_train): 0 and NULL here", who);
  } else if (loss->opacity_weight > 0.0f) {
    RTXN_REQUIRE(vr_mode != RTXN_VR_COMPAT, "%s: loss->opacity_weight > 0 needs the RTXN_VR_NERF compositor, not RTXN_VR_COMPAT", who);
    RTXN_REQUIRE(target_channels == 4, "%s: loss->opacity_weight > 0 needs 4-channel (RGBA) targets: alpha is the target's fourth channel", who);
  }
  RTXN_REQUIRE(!(loss->opacity && vr_mode == RTXN_VR_COMPAT),
               "%s: loss->opacity is written by the RTXN_VR_NERF compositor only, not with RTXN_VR_COMPAT", who);
  *active = !(loss->kind == RTXN_LOSS_L2 && loss->opacity_weight == 0.0f && !loss->opacity);
  return RTXN_OK;
}

int rtxn::check_train_regularizer(const rtxn_train_regularizer* reg, int vr_mode, int sample_type, const char* who, bool* active) {
  *active = false;
  if (!reg) return RTXN_OK;
  RTXN_REQUIRE(std::isfinite(reg->distortion_weight) && reg->distortion_weight >= 0.0f, "%s: reg->distortion_weight = %g (finite, >= 0)", who,
               (double)reg->distortion_weight);
  if (!(reg->distortion_weight > 0.0f || reg->distortion || reg->depth)) return RTXN_OK;
  RTXN_REQUIRE(reg->t_start && reg->t_end,
               "%s: reg->t_start / reg->t_end are NULL: the distortion term and its outputs need the segments' entry and exit distances", who);
  RTXN_REQUIRE(vr_mode == RTXN_VR_NERF, "%s: reg->distortion_weight / distortion / depth need the RTXN_VR_NERF compositor (vr_mode = %d)", who,
               vr_mode);
  RTXN_REQUIRE(sample_type < 0 || sample_type == RTXN_SAMPLING_MIDPOINT_WORLD || sample_type == RTXN_SAMPLING_JITTER_WORLD,
               "%s: reg->distortion_weight / distortion / depth need sample_type RTXN_SAMPLING_MIDPOINT_WORLD or _JITTER_WORLD (sample_type = %d): "
               "distances are world units along the ray", who, sample_type);
  *active = true;
  return RTXN_OK;
}

int rtxn::check_train_depth(const rtxn_train_depth* depth, const rtxn_train_regularizer* reg, const rtxn_ray_gradients* rays, int vr_mode,
                            int sample_type, const char* who, bool* active) {
  *active = false;
  if (!depth) return RTXN_OK;
  RTXN_REQUIRE(std::isfinite(depth->weight) && depth->weight >= 0.0f, "%s: depth->weight = %g (finite, >= 0)", who, (double)depth->weight);
  RTXN_REQUIRE(depth->kind == RTXN_LOSS_L2 || depth->kind == RTXN_LOSS_L1 || depth->kind == RTXN_LOSS_HUBER,
               "%s: depth->kind = %d: unknown depth loss kind (RTXN_LOSS_L2 | _L1 | _HUBER)", who, depth->kind);
  if (depth->kind == RTXN_LOSS_HUBER)
    RTXN_REQUIRE(std::isfinite(depth->param) && depth->param > 0.0f, "%s: depth->param = %g: RTXN_LOSS_HUBER needs a finite delta > 0", who,
                 (double)depth->param);
  if (!(depth->weight > 0.0f || depth->depth || depth->depth_loss)) return RTXN_OK;
  RTXN_REQUIRE(depth->target, "%s: depth->target is NULL: the depth term and its outputs need the rays' depth targets", who);
  RTXN_REQUIRE(depth->t_start && depth->t_end,
               "%s: depth->t_start / depth->t_end are NULL: the depth term and its outputs need the segments' entry and exit distances", who);
  RTXN_REQUIRE(vr_mode == RTXN_VR_NERF, "%s: depth->weight / depth / depth_loss need the RTXN_VR_NERF compositor (vr_mode = %d)", who, vr_mode);
  RTXN_REQUIRE(sample_type < 0 || sample_type == RTXN_SAMPLING_MIDPOINT_WORLD || sample_type == RTXN_SAMPLING_JITTER_WORLD,
               "%s: depth->weight / depth / depth_loss need sample_type RTXN_SAMPLING_MIDPOINT_WORLD or _JITTER_WORLD (sample_type = %d): "
               "distances are world units along the ray", who, sample_type);
  RTXN_REQUIRE(!reg || !reg->t_start || (reg->t_start == depth->t_start && reg->t_end == depth->t_end),
               "%s: depth->t_start / t_end and reg->t_start / t_end must be the same buffers (the traversal writes them once)", who);
  RTXN_REQUIRE(!rays || (rays->t_start == depth->t_start && rays->t_end == depth->t_end),
               "%s: rays->t_start / t_end and depth->t_start / t_end must be the same buffers (the traversal writes them once)", who);
  *active = true;
  return RTXN_OK;
}

extern "C" int rtxn_volrender_loss_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                                         int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                                         void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                                         const rtxn_train_background* bg, const rtxn_train_loss* loss, rtxn_stream_t stream) {
  return rtxn::composite_train("rtxn_volrender_loss_train", {network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target,
                               loss_scale, pixels, loss_gradients_half, loss_sum, radiance_gradients}, bg, loss, nullptr, nullptr, stream);
}

extern "C" int rtxn_volrender_reg_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                                        int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                                        void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                                        const rtxn_train_background* bg, const rtxn_train_loss* loss, const rtxn_train_regularizer* reg,
                                        rtxn_stream_t stream) {
  return rtxn::composite_train("rtxn_volrender_reg_train", {network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target,
                               loss_scale, pixels, loss_gradients_half, loss_sum, radiance_gradients}, bg, loss, reg, nullptr, stream);
}

// the loss scale read from the scaler's device word (loss_scale is not read); scaler == NULL: rtxn_volrender_reg_train
extern "C" int rtxn_volrender_scaled_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                                           int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                                           void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                                           const rtxn_train_background* bg, const rtxn_train_loss* loss, const rtxn_train_regularizer* reg,
                                           const rtxn_loss_scaler* scaler, rtxn_stream_t stream) {
  const char* who = scaler ? "rtxn_volrender_scaled_train" : "rtxn_volrender_reg_train";
  if (scaler) {
    const int rc = rtxn::check_loss_scaler(scaler, who, true);
    if (rc != RTXN_OK) return rc;
  }
  return rtxn::composite_train(who, {network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target,
                               scaler ? 0.0f : loss_scale, pixels, loss_gradients_half, loss_sum, radiance_gradients}, bg, loss, reg,
                               scaler ? &scaler->state->scale : nullptr, stream);
}

// the depth term beside everything below it; scaler as rtxn_volrender_scaled_train's; depth == NULL or inactive: that call
extern "C" int rtxn_volrender_depth_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                                          int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                                          void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                                          const rtxn_train_background* bg, const rtxn_train_loss* loss, const rtxn_train_regularizer* reg,
                                          const rtxn_loss_scaler* scaler, const rtxn_train_depth* depth, rtxn_stream_t stream) {
  const char* who = depth ? "rtxn_volrender_depth_train" : scaler ? "rtxn_volrender_scaled_train" : "rtxn_volrender_reg_train";
  if (scaler) {
    const int rc = rtxn::check_loss_scaler(scaler, who, true);
    if (rc != RTXN_OK) return rc;
  }
  return rtxn::composite_train(who, {network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target,
                               scaler ? 0.0f : loss_scale, pixels, loss_gradients_half, loss_sum, radiance_gradients}, bg, loss, reg,
                               scaler ? &scaler->state->scale : nullptr, stream, depth);
}
