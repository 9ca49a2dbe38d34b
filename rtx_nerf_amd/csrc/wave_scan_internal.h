// The compositors' wave-wide scan helpers and the fp16 gradient record, shared by volrender.hip, terminate.hip and
// composite_train.hip.  Internal to librtxn.so.  Anonymous namespace: every helper is inlined, and the kernels that take
// half4 pointers carry its name in their symbols, which tests/test_compositor_isa.py pins.
#pragma once
#include "common.h"

namespace {

// Inclusive prefix sum over the 64 lanes in six DPP adds (row_shr 1/2/4/8 inside each row of 16, then row_bcast:15 into rows
// 1 and 3 and row_bcast:31 into rows 2 and 3): no LDS crossbar round trips -- the __shfl_up form (six dependent
// ds_bpermute_b32) was most of a compositor step's latency (tools/probe/dpp_scan_probe.hip checks the lane pattern).
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

// Sum over the wave, returned in every lane: the DPP inclusive scan above leaves the total in lane 63, read back as a scalar
// (six VALU adds + v_readlane; the __shfl_xor butterfly was six dependent ds_swizzle / ds_bpermute round trips, three times
// per ray in the compositors).
__device__ __forceinline__ float wave_sum(float v) { return lane63(wave_incl_scan_f(v)); }
// lane - 1's value (lane 0: 0): DPP wave_shr:1
__device__ __forceinline__ float lane_below(float v) { return dpp_term<0x138, 0xf>(v); }

// The same sum for a double, the two words of each value moved by the same DPP pattern (a row or lane the pattern does not
// reach reads both words as 0, i.e. +0.0): a fixed order, the same in every launch.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_term_d(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, 0xf, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xf, true);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum_d(double v) {
  v += dpp_term_d<0x111, 0xf>(v);
  v += dpp_term_d<0x112, 0xf>(v);
  v += dpp_term_d<0x114, 0xf>(v);
  v += dpp_term_d<0x118, 0xf>(v);
  v += dpp_term_d<0x142, 0xa>(v);
  v += dpp_term_d<0x143, 0xc>(v);
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 63);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

struct alignas(8) half4 {
  __half x, y, z, w;
};

}  // namespace
