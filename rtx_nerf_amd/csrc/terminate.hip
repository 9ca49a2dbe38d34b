// Early ray termination for the frame entry (rtxn_render_set_termination): the kernels of one ROUND.
//
// A frame with termination shades its rays front to back in N rounds instead of all at once.  Round k takes the next
// s0 * 2^k segments of every ray still alive (the last round: all that remain), copies their records into a packed round
// scratch, runs the UNCHANGED fused MLP entry point on that scratch, and continues each ray's compositing sum from the state
// the previous round left.  A ray whose optical depth T exceeds t_stop = -log(eps) at a round boundary is not shaded further:
// both compositing modes bound everything behind optical depth T by exp(-T), so the pixel moves by at most eps.
// Every count -- what a ray takes, where its records lie in the scratch, how many segments the round has -- stays in device
// memory: render.hip enqueues all N rounds back to back without reading anything, so the frame stays hipGraph-capturable.
//
//   term_begin_kernel    round 0's selection: take = min(num_stored, quota), done = 0
//   (rtxn_scan_hits)     off = exclusive scan of take, round_total[k] = its sum
//   term_gather_kernel   CSR records [indices + done, +take) -> scratch [off, +take)
//   (the MLP entry)      radiance (and the NERF step) of the scratch's round_total[k] segments
//   term_resume_kernel   one wave per ray: load the carried state, composite take * 32 samples, then store the state and
//                        SELECT the next round's take, or write the ray's outputs in the last round it is in
//   term_account_kernel  one thread: the frame's shaded / total segments into 64-bit per-slot counters
//
// The compositing arithmetic is that of volrender.hip's one-sample forward body (fwd_body<MODE, COMPACT = true, AUX = true>),
// restated here rather than shared: that file's kernels are pinned by their machine code (tests/test_compositor_isa.py), and
// a body inlined into one more kernel is optimised once more.  The wave scan helpers and half4 are shared
// (wave_scan_internal.h): they are inlined everywhere and leave every kernel's code as it was.  Sums are reduced over the wave at every round boundary instead
// of once per ray, so against the plain compositors the results agree to fp32 summation order, not bit for bit.
#include "terminate_internal.h"
#include "wave_scan_internal.h"

namespace {

constexpr int K = RTXN_NUM_SAMPLES_PER_SEGMENT;   // 32: a 64-lane step is two whole segments
static_assert(K == 32, "the resume kernel's index arithmetic assumes 32 samples per segment");

struct F3 {       // a float3 record: 12 bytes, 4-byte aligned, moved as one global_load/store_dwordx3
  float x, y, z;
};

__global__ __launch_bounds__(256) void term_begin_kernel(const int* __restrict__ num_stored, int n_rays, int quota,
                                                         int* __restrict__ take, int* __restrict__ done) {
  const int ray = blockIdx.x * 256 + threadIdx.x;
  if (ray >= n_rays) return;
  const int ns = num_stored[ray];
  take[ray] = ns < quota ? ns : quota;
  done[ray] = 0;
}

// A wave owns 64 consecutive rays and copies their records with every lane busy: the rays' takes are scanned over the wave,
// the wave's records numbered 0 .. total-1, and lane l of each step of 64 finds the ray of record f = f0 + l by bisection
// over the inclusive sums (six ds_bpermute).  A record is 32 B (+8 with t_start / t_end) against ~8 MFLOP of shading, hence a
// copy and not an indirection inside the MLP kernels.
template <bool AUX>
__global__ __launch_bounds__(256) void term_gather_kernel(const int* __restrict__ take, const int* __restrict__ off,
                                                          const int* __restrict__ done, const int* __restrict__ indices, int n_rays,
                                                          long capacity, const F3* __restrict__ start, const F3* __restrict__ end,
                                                          const float2* __restrict__ seg_view, const float* __restrict__ t_start,
                                                          const float* __restrict__ t_end, F3* __restrict__ o_start,
                                                          F3* __restrict__ o_end, float2* __restrict__ o_view,
                                                          float* __restrict__ o_t_start, float* __restrict__ o_t_end) {
  const int lane = threadIdx.x & 63;
  const int ray0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (ray0 >= n_rays) return;                           // wave-uniform
  const int ray = ray0 + lane;
  int tk = 0, dst0 = 0, src0 = 0;
  if (ray < n_rays) {
    tk = take[ray];
    if (tk > 0) {
      dst0 = off[ray];
      src0 = indices[ray] + done[ray];
    }
  }
  int incl = tk;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  const int excl = incl - tk;
  const int total = __shfl(incl, 63, 64);
  for (int f0 = 0; f0 < total; f0 += 64) {
    const int f = f0 + lane;
    int lo = 0, hi = 63;                                // the first lane whose inclusive sum exceeds f owns record f
#pragma unroll
    for (int it = 0; it < 6; ++it) {
      const int mid = (lo + hi) >> 1;
      const int v = __shfl(incl, mid, 64);
      if (v > f) hi = mid;
      else lo = mid + 1;
    }
    lo = lo > 63 ? 63 : lo;                             // lanes beyond the wave's last record: masked below
    const int j = f - __shfl(excl, lo, 64);
    const long src = (long)__shfl(src0, lo, 64) + j;
    const long dst = (long)__shfl(dst0, lo, 64) + j;
    if (f < total && j >= 0 && src >= 0 && src < capacity && dst >= 0 && dst < capacity) {
      o_start[dst] = start[src];
      o_end[dst] = end[src];
      o_view[dst] = seg_view[src];
      if (AUX) {
        o_t_start[dst] = t_start[src];
        o_t_end[dst] = t_end[src];
      }
    }
  }
}

// A wave takes kRaysPerWave consecutive rays one after the other: most rays of a frame hit nothing, and from the second round
// on most of the rest are finished, so a wave per ray would make every round's launch a matter of wave turnover.
constexpr int kRaysPerWave = 8;

struct ResumeArgs {
  const half4* radiance;      // the round scratch
  const float* seg_step;      // RTXN_VR_NERF
  const float* t_start;       // depth only
  const float* t_end;
  const int* num_stored;
  const int* off;
  int* take;
  int* done;
  float4* state;
  int n_rays;
  int first;                  // round 0: no state to load; rays without segments get their (empty) outputs here
  int next_quota;             // segments a surviving ray takes next round
  float t_stop;
  float u0;
  rtxn::TermOutputs out;
};

template <int MODE>
__global__ __launch_bounds__(256) void term_resume_kernel(ResumeArgs a) {
  const int lane = threadIdx.x & 63;
  const int ray0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * kRaysPerWave;
  const bool want_depth = a.out.depth != nullptr;
  for (int q = 0; q < kRaysPerWave; ++q) {
    const int ray = ray0 + q;
    if (ray >= a.n_rays) return;
    const int tk = a.take[ray];
    if (tk <= 0) {
      // never in a round (no stored segment): opacity 0, depth 0, pixel = background.  Rays that finished in an earlier
      // round wrote their outputs there.
      if (a.first && lane == 0) {
        a.out.pixels[3 * (long)ray] = a.out.bg[0];
        a.out.pixels[3 * (long)ray + 1] = a.out.bg[1];
        a.out.pixels[3 * (long)ray + 2] = a.out.bg[2];
        if (a.out.opacity) a.out.opacity[ray] = 0.0f;
        if (want_depth) a.out.depth[ray] = 0.0f;
      }
      continue;
    }
    const int seg0 = a.off[ray], dn = a.done[ray], ns = a.num_stored[ray];
    float T_carry = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sd = 0.0f;
    if (!a.first) {
      const float4 s0 = a.state[2 * (long)ray], s1 = a.state[2 * (long)ray + 1];
      T_carry = s0.x; sr = s0.y; sg = s0.z; sb = s0.w;
      sw = s1.x; sd = s1.y;
    }
    // COMPAT: delta_i = |t_i - t_{i-1}| is not reset at a segment boundary, and with the implicit REGULAR t_vals the sample
    // before a segment's first is the previous segment's last, t = 1 (the ray's very first sample: t_{-1} = 0)
    float t_carry = dn > 0 ? 1.0f : 0.0f;
    const int n = tk * K;
    const long base = (long)seg0 * K;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f, ad = 0.0f;
    for (int s0 = 0; s0 < n; s0 += 64) {
      const bool act = s0 + lane < n;
      float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
      float t = 0.0f, d = 0.0f;
      if (act) {
        const half4 c16 = a.radiance[base + s0 + lane];
        c = make_float4(__half2float(c16.x), __half2float(c16.y), __half2float(c16.z), __half2float(c16.w));
        const int j = seg0 + ((s0 + lane) >> 5);
        if (MODE == RTXN_VR_COMPAT) t = (float)((lane & (K - 1)) + 1) * (1.0f / (float)K);
        else t = a.seg_step[j];
        if (want_depth) {
          const float ts = a.t_start[j], te = a.t_end[j];
          d = fmaf(((float)(lane & (K - 1)) + a.u0) * (1.0f / (float)K), te - ts, ts);
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
        t_carry = lane63(t);      // inactive lanes only occur in a round's final step
      } else {
        x = act ? t * c.w : 0.0f;
        const float incl = wave_incl_scan_f(x);
        const float T_excl = T_carry + incl - x;
        w = act ? expf(-T_excl) * (1.0f - expf(-x)) : 0.0f;
        T_carry += lane63(incl);
      }
      ar = fmaf(w, c.x, ar);
      ag = fmaf(w, c.y, ag);
      ab = fmaf(w, c.z, ab);
      aw += w;
      ad = fmaf(w, d, ad);
    }
    sr += wave_sum(ar);
    sg += wave_sum(ag);
    sb += wave_sum(ab);
    sw += wave_sum(aw);
    if (want_depth) sd += wave_sum(ad);
    // the round boundary: alive iff segments are left and the optical depth has not passed t_stop (the last round's quota
    // is everything, so nothing is left after it)
    const int dn2 = dn + tk;
    const bool alive = dn2 < ns && T_carry <= a.t_stop;
    if (lane == 0) {
      a.done[ray] = dn2;
      const int left = ns - dn2;
      a.take[ray] = alive ? (left < a.next_quota ? left : a.next_quota) : 0;
      if (alive) {
        a.state[2 * (long)ray] = make_float4(T_carry, sr, sg, sb);
        a.state[2 * (long)ray + 1] = make_float4(sw, sd, 0.0f, 0.0f);
      } else {
        const float rest = 1.0f - sw;
        if (a.out.bg[0] != 0.0f) sr = fmaf(rest, a.out.bg[0], sr);
        if (a.out.bg[1] != 0.0f) sg = fmaf(rest, a.out.bg[1], sg);
        if (a.out.bg[2] != 0.0f) sb = fmaf(rest, a.out.bg[2], sb);
        a.out.pixels[3 * (long)ray] = sr;
        a.out.pixels[3 * (long)ray + 1] = sg;
        a.out.pixels[3 * (long)ray + 2] = sb;
        if (a.out.opacity) a.out.opacity[ray] = sw;
        if (want_depth) a.out.depth[ray] = sd;
      }
    }
  }
}

// {frames, shaded and total segments of the last frame, cumulative shaded and total}: cumulative on the device, so a replayed
// hipGraph counts itself (as frame_account_kernel in render.hip)
__global__ void term_account_kernel(const int* __restrict__ round_total, int n_rounds, const int* __restrict__ total, int capacity,
                                    long* __restrict__ acct) {
  long shaded = 0;
  for (int k = 0; k < n_rounds; ++k) shaded += round_total[k];
  const int t = *total;
  const long stored = t < capacity ? t : capacity;
  acct[0] += 1;
  acct[1] = shaded;
  acct[2] = stored;
  acct[3] += shaded;
  acct[4] += stored;
}

}  // namespace

namespace rtxn {

int term_begin(const int* num_stored, int n_rays, int quota, const TermBuffers& b, hipStream_t s) {
  term_begin_kernel<<<(n_rays + 255) / 256, 256, 0, s>>>(num_stored, n_rays, quota, b.take, b.done);
  RTXN_LAUNCH_CHECK("term_begin_kernel");
  return RTXN_OK;
}

int term_gather(const TermBuffers& b, const int* indices, int n_rays, long capacity, const float* start, const float* end,
                const float* seg_view, const float* t_start, const float* t_end, hipStream_t s) {
  const int grid = (n_rays + 255) / 256;                // 4 waves x 64 rays per block
  const F3* st = reinterpret_cast<const F3*>(start);
  const F3* en = reinterpret_cast<const F3*>(end);
  const float2* vw = reinterpret_cast<const float2*>(seg_view);
  F3* ost = reinterpret_cast<F3*>(b.start);
  F3* oen = reinterpret_cast<F3*>(b.end);
  float2* ovw = reinterpret_cast<float2*>(b.seg_view);
  if (t_start && t_end && b.t_start && b.t_end)
    term_gather_kernel<true><<<grid, 256, 0, s>>>(b.take, b.off, b.done, indices, n_rays, capacity, st, en, vw, t_start, t_end, ost, oen, ovw,
                                                  b.t_start, b.t_end);
  else
    term_gather_kernel<false><<<grid, 256, 0, s>>>(b.take, b.off, b.done, indices, n_rays, capacity, st, en, vw, nullptr, nullptr, ost, oen,
                                                   ovw, nullptr, nullptr);
  RTXN_LAUNCH_CHECK("term_gather_kernel");
  return RTXN_OK;
}

int term_resume(const TermBuffers& b, const int* num_stored, int n_rays, int vr_mode, float u0, bool first, int next_quota,
                float t_stop, const TermOutputs& o, hipStream_t s) {
  ResumeArgs a;
  a.radiance = static_cast<const half4*>(b.radiance);
  a.seg_step = b.seg_step;
  a.t_start = b.t_start;
  a.t_end = b.t_end;
  a.num_stored = num_stored;
  a.off = b.off;
  a.take = b.take;
  a.done = b.done;
  a.state = b.state;
  a.n_rays = n_rays;
  a.first = first ? 1 : 0;
  a.next_quota = next_quota;
  a.t_stop = t_stop;
  a.u0 = u0;
  a.out = o;
  if (a.out.depth && !(a.t_start && a.t_end)) a.out.depth = nullptr;    // refused earlier (check_outputs); never read NULL
  const int grid = (n_rays + 4 * kRaysPerWave - 1) / (4 * kRaysPerWave);
  if (vr_mode == RTXN_VR_NERF) {
    RTXN_REQUIRE(a.seg_step != nullptr, "term_resume: RTXN_VR_NERF without the segments' step lengths");
    term_resume_kernel<RTXN_VR_NERF><<<grid, 256, 0, s>>>(a);
  } else {
    term_resume_kernel<RTXN_VR_COMPAT><<<grid, 256, 0, s>>>(a);
  }
  RTXN_LAUNCH_CHECK("term_resume_kernel");
  return RTXN_OK;
}

int term_account(const TermBuffers& b, int n_rounds, const int* total, int capacity, hipStream_t s) {
  term_account_kernel<<<1, 1, 0, s>>>(b.round_total, n_rounds, total, capacity, b.acct);
  RTXN_LAUNCH_CHECK("term_account_kernel");
  RTXN_HIP(hipMemcpyAsync(b.acct_host, b.acct, 5 * sizeof(long), hipMemcpyDeviceToHost, s));
  return RTXN_OK;
}

}  // namespace rtxn
