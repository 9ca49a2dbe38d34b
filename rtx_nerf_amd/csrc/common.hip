// Error plumbing, per-device launch helpers and version of librtxn.so.
#include "common.h"

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <vector>

namespace rtxn {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int fail_hip(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
  return RTXN_ERR_HIP;
}

int require_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device available (librtxn has no CPU fallback)");
    return RTXN_ERR_HIP;
  }
  return RTXN_OK;
}

const char* last_error() { return g_err; }

static __global__ void zero_words_kernel(unsigned* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}

hipError_t zero_words(void* p, size_t n_words, hipStream_t stream) {
  if (n_words == 0) return hipSuccess;
  const size_t blocks = (n_words + 255) / 256;
  zero_words_kernel<<<(unsigned)(blocks > 1024 ? 1024 : blocks), 256, 0, stream>>>(static_cast<unsigned*>(p), n_words);
  return hipGetLastError();
}

hipError_t cu_count(int* n_cu) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess && *n_cu <= 0) *n_cu = 256;
  return e;
}

hipError_t set_lds_once(const void* fn, size_t bytes) {
  struct Seen { int dev; const void* fn; size_t bytes; };
  static std::mutex mu;
  static std::vector<Seen> seen;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  for (Seen& q : seen)
    if (q.dev == dev && q.fn == fn) {
      if (q.bytes >= bytes) return hipSuccess;
      e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (e == hipSuccess) q.bytes = bytes;
      return e;
    }
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) seen.push_back(Seen{dev, fn, bytes});
  return e;
}

int check_sample_jitter(const char* who, int sample_type, const rtxn_sample_jitter* jitter, int vr_mode) {
  RTXN_REQUIRE(sample_type != RTXN_SAMPLING_JITTER_WORLD || jitter, "%s: RTXN_SAMPLING_JITTER_WORLD needs a jitter struct (seed, step)", who);
  RTXN_REQUIRE(!jitter || sample_type == RTXN_SAMPLING_JITTER_WORLD,
               "%s: a jitter struct with sample_type %d (it goes with RTXN_SAMPLING_JITTER_WORLD only; pass NULL otherwise)", who, sample_type);
  RTXN_REQUIRE(!jitter || vr_mode != RTXN_VR_COMPAT,
               "%s: RTXN_SAMPLING_JITTER_WORLD with RTXN_VR_COMPAT (its t_vals are step lengths, which that compositor does not take)", who);
  return RTXN_OK;
}

}  // namespace rtxn

extern "C" int rtxn_version(void) { return RTXN_VERSION; }
extern "C" const char* rtxn_last_error(void) { return rtxn::last_error(); }
