// The training compositor for the losses of rtxn_train_loss (include/rtxn.h): rtxn_volrender_l2_train_ex's two
// sweeps with the per-ray step between them -- pixel, loss value, fp16 loss gradient -- evaluated by loss_internal.h's
// loss_term instead of the hard-wired L2, plus the alpha term lambda (A - alpha)^2, whose gradient g_A enters the second sweep
// as one more constant beside the background's dot product:
//   dL/dw_k = g.c_k - g.b + g_A,   S = g.(sum w c) - (g.b) A + g_A A.
// A translation unit of its own: tests/test_compositor_isa.py pins the machine code of every volrender_ device function, and
// a body shared with them by inlining changes their bytes, so these kernels are copies of volrender_l2_bg_kernel
// and volrender_l2_bg_multi_kernel<4> (volrender.hip) -- schedule and per-sample arithmetic operation for operation -- under
// names of their own, with copies of the small scan helpers, as terminate.hip has.  Loss kind, parameter, lambda and the
// background flag are wave-uniform values of an argument struct; the loss is evaluated once per ray on three channels, so the
// kernels are not instantiated per kind.
#include <cmath>

#include "background_internal.h"
#include "common.h"
#include "loss_internal.h"

namespace {

// volrender.hip's DPP scan helpers (copies; tools/probe/dpp_scan_probe.hip checks the lane pattern)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_term(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ float wave_incl_scan_f(float v) {
  v += dpp_term<0x111, 0xf>(v);
  v += dpp_term<0x112, 0xf>(v);
  v += dpp_term<0x114, 0xf>(v);
  v += dpp_term<0x118, 0xf>(v);
  v += dpp_term<0x142, 0xa>(v);
  v += dpp_term<0x143, 0xc>(v);
  return v;
}
__device__ __forceinline__ float lane63(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_sum(float v) { return lane63(wave_incl_scan_f(v)); }

struct alignas(8) half4 {
  __half x, y, z, w;
};

// What a ray's wave does between the sweeps: pixel, loss gradient (fp16, stored and handed on in that form), the ray's share of
// the loss; returns it.  Every value is wave-uniform; lane 0 stores.
struct RayGrad {
  float g0, g1, g2, gA;
};
__device__ __forceinline__ float ray_step(const BgArgs& bga, const LossArgs& la, const float* __restrict__ target, int ray, int batch_size,
                                          int lane, float loss_scale, float ar, float ag, float ab, float aw, float* __restrict__ pixels,
                                          __half* __restrict__ loss_gradients, float (&bg)[3], RayGrad& g) {
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
  const float value = ray_loss_term(la, p, tg, aw, alpha, inv_n, inv_rays, dl, dA);
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
  }
  return value;
}

// one ray per wave, 64 samples per step: the form for odd K or misaligned buffers (volrender_l2_bg_kernel's schedule)
__global__ __launch_bounds__(256) void composite_loss_kernel(const float4* __restrict__ radiance, const float* __restrict__ step_len,
                                                             const int* __restrict__ num_hits, const int* __restrict__ indices,
                                                             int batch_size, int K, const float* __restrict__ target,
                                                             float loss_scale, float* __restrict__ pixels,
                                                             __half* __restrict__ loss_gradients, float* __restrict__ loss_sum,
                                                             half4* __restrict__ grads, BgArgs bga, LossArgs la) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= batch_size) return;
  const long base = (long)indices[ray] * K;
  const long n = (long)num_hits[ray] * K;
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
  float bg[3];
  RayGrad g;
  const float value = ray_step(bga, la, target, ray, batch_size, lane, loss_scale, ar, ag, ab, aw, pixels, loss_gradients, bg, g);
  if (lane == 0 && loss_sum) atomicAdd(loss_sum, value);
  const float g0 = g.g0, g1 = g.g1, g2 = g.g2;
  const float gbg = g0 * bg[0] + g1 * bg[1] + g2 * bg[2];
  const float S = ((g0 * ar + g1 * ag + g2 * ab) - gbg * aw) + g.gA * aw;     // = sum_k w_k (g . (c_k - bg) + g_A)
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
    const float gc = ((g0 * c.x + g1 * c.y + g2 * c.z) - gbg) + g.gA;
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

// U blocks of 128 samples per step, two per lane (volrender_l2_bg_multi_kernel's schedule and arithmetic): even K, 8-byte
// aligned step lengths, 16-byte aligned gradients.  The loss is reduced per block and added once per block at the very end.
template <int U>
__global__ __launch_bounds__(256) void composite_loss_multi_kernel(const float4* __restrict__ radiance, const float* __restrict__ step_len,
                                                                   const int* __restrict__ num_hits, const int* __restrict__ indices,
                                                                   int batch_size, int K, const float* __restrict__ target,
                                                                   float loss_scale, float* __restrict__ pixels,
                                                                   __half* __restrict__ loss_gradients, float* __restrict__ loss_sum,
                                                                   half4* __restrict__ grads, BgArgs bga, LossArgs la) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ray = blockIdx.x * 4 + wave;
  float loss_part = 0.0f;
  if (ray < batch_size) {
    const long base = (long)indices[ray] * K;
    const long n = (long)num_hits[ray] * K;          // even
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
    float bg[3];
    RayGrad g;
    loss_part = ray_step(bga, la, target, ray, batch_size, lane, loss_scale, ar, ag, ab, aw, pixels, loss_gradients, bg, g);
    const float g0 = g.g0, g1 = g.g1, g2 = g.g2;
    const float gbg = g0 * bg[0] + g1 * bg[1] + g2 * bg[2];
    const float S = ((g0 * ar + g1 * ag + g2 * ab) - gbg * aw) + g.gA * aw;     // = sum_k w_k (g . (c_k - bg) + g_A)
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
        gc0[u] = ((g0 * cur[u].c0.x + g1 * cur[u].c0.y + g2 * cur[u].c0.z) - gbg) + g.gA;
        gc1[u] = ((g0 * cur[u].c1.x + g1 * cur[u].c1.y + g2 * cur[u].c1.z) - gbg) + g.gA;
        // inactive lanes: Ti (1 - ex) = 0 (x = 0), so the constants of their zero colour add nothing to the prefix
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

extern "C" int rtxn_volrender_loss_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                                         int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                                         void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                                         const rtxn_train_background* bg, const rtxn_train_loss* loss, rtxn_stream_t stream) {
  const char* who = "rtxn_volrender_loss_train";
  bool bg_active = false, loss_active = false;
  int rc = rtxn::check_train_background(bg, RTXN_VR_NERF, who, &bg_active);
  if (rc != RTXN_OK) return rc;
  rc = rtxn::check_train_loss(loss, bg_active ? bg->target_channels : 3, RTXN_VR_NERF, who, &loss_active);
  if (rc != RTXN_OK) return rc;
  if (!loss_active)      // exactly what the entry point without the struct runs
    return rtxn_volrender_l2_train_ex(network_outputs, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale, pixels,
                                      loss_gradients_half, loss_sum, radiance_gradients, bg, stream);
  RTXN_REQUIRE(batch_size >= 0, "%s: batch_size = %d < 0", who, batch_size);
  RTXN_REQUIRE(num_samples_per_hit > 0, "%s: num_samples_per_hit = %d", who, num_samples_per_hit);
  // deterministic mode: the kernels get no loss pointer (their sum is float atomics); loss.hip sums behind them
  const bool det_loss = loss_sum && batch_size > 0 && rtxn::deterministic_mode();
  RTXN_REQUIRE(!(det_loss && loss->opacity_weight > 0.0f && !loss->opacity),
               "%s: loss->opacity is NULL: in deterministic mode the alpha term of the loss is summed from the opacities the compositor writes there",
               who);
  RTXN_DEVICE_OR_FAIL();
  hipStream_t s = rtxn::as_stream(stream);
  if (loss_sum && !det_loss) RTXN_HIP(rtxn::zero_words(loss_sum, 1, s));
  if (batch_size == 0) return RTXN_OK;
  RTXN_REQUIRE(network_outputs && ray_hit && num_hits && indices && target && pixels && radiance_gradients, "%s: NULL buffer", who);
  RTXN_REQUIRE(((uintptr_t)network_outputs & 15) == 0 && ((uintptr_t)radiance_gradients & 7) == 0,
               "%s: radiance must be 16-byte and gradients 8-byte aligned", who);
  BgArgs a{};
  a.mode = RTXN_BG_NONE;
  a.target_channels = 3;
  if (bg_active) {
    a.mode = bg->mode;
    for (int c = 0; c < 3; ++c) a.color[c] = bg->color[c];
    a.seed = bg->seed;
    a.step = bg->step;
    a.target_channels = bg->target_channels;
  }
  LossArgs la{};
  la.kind = loss->kind;
  la.param = loss->param;
  la.opacity_weight = loss->opacity_weight;
  la.has_background = bg_active ? 1 : 0;
  la.opacity = loss->opacity;
  // 512 samples per step, two per lane: an even K, 8-byte-aligned step lengths and 16-byte-aligned gradients
  const bool pairs = num_samples_per_hit % 2 == 0 && ((uintptr_t)ray_hit & 7) == 0 && ((uintptr_t)radiance_gradients & 15) == 0;
  const dim3 grid((batch_size + 3) / 4), block(256);
  const float4* rad = reinterpret_cast<const float4*>(network_outputs);
  __half* lg = static_cast<__half*>(loss_gradients_half);
  half4* out = static_cast<half4*>(radiance_gradients);
  float* const kernel_sum = det_loss ? nullptr : loss_sum;
  if (pairs)
    composite_loss_multi_kernel<4><<<grid, block, 0, s>>>(rad, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale,
                                                          pixels, lg, kernel_sum, out, a, la);
  else
    composite_loss_kernel<<<grid, block, 0, s>>>(rad, ray_hit, num_hits, indices, batch_size, num_samples_per_hit, target, loss_scale, pixels,
                                                 lg, kernel_sum, out, a, la);
  RTXN_LAUNCH_CHECK("composite_loss_kernel");
  if (det_loss) return rtxn::loss_fixed_order(pixels, target, batch_size, bg_active ? bg : nullptr, loss, loss_sum, s);
  return RTXN_OK;
}
