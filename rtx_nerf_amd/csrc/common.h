// Shared host-side helpers of librtxn.so (error reporting, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "rtxn.h"

namespace rtxn {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int fail_hip(hipError_t e, const char* what);

inline hipStream_t as_stream(rtxn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// The library has no CPU path: every compute entry point goes through this.
int require_device();

// Zeroes n_words 32-bit words with a KERNEL.  Not hipMemsetAsync: as a memset node of a captured hipGraph it filled the 4 bytes
// of a loss sum with a stray byte (0xE8E8E8E8, 0x78787878, ...) on the graph's FIRST launch and with zeros from the second on
// (ROCm 7.2, round 3: tools/probe/captured_loss_dbg.py, profiles/r03/graph_memset_first_launch.txt), so nothing on a capturable
// path uses it any more.
hipError_t zero_words(void* p, size_t n_words, hipStream_t stream);

// Per-device launch helpers (a process may drive several GPUs, and they need not be alike).  Library-internal: hidden, so the
// exported symbol list stays the C ABI's.
// Compute units of the current device, for the persistent grids; 256 where the runtime reports none.
__attribute__((visibility("hidden"))) hipError_t cu_count(int* n_cu);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel), again only for a larger size: not repeated in front
// of every launch, and never inside a stream capture after the first, un-captured, call.
__attribute__((visibility("hidden"))) hipError_t set_lds_once(const void* fn, size_t bytes);

// Deterministic mode (rtxn_set_deterministic_workspace, train.hip): whether a fixed-point shadow is registered right now.
__attribute__((visibility("hidden"))) bool deterministic_mode();
// ... in which the training compositor's loss scalar is summed in a fixed order behind the compositor instead of by its float
// atomics (loss.hip): *loss_sum = the L2 loss of pixels float[n_rays][3] against target float[n_rays][target_channels], a
// 4-channel target composited over the ray's background (bg_mode rtxn_train_background_mode, bg_color host float[3] or NULL).
__attribute__((visibility("hidden"))) int l2_loss_fixed_order(const float* pixels, const float* target, int n_rays, int bg_mode,
                                                              const float* bg_color, unsigned bg_seed, const int* bg_step,
                                                              int target_channels, float* loss_sum, hipStream_t stream);

// The rules of a training background (rtxn_train_background, include/rtxn.h), host only: RTXN_ERR_INVALID with a message, or
// RTXN_OK with *active = whether a background is composited at all.
int check_train_background(const rtxn_train_background* bg, int vr_mode, const char* who, bool* active);

// The rules of a training loss (rtxn_train_loss, include/rtxn.h), host only, composite_train.hip: RTXN_ERR_INVALID with
// a message naming the field, or RTXN_OK with *active = whether the loss kernels run at all (NULL, or L2 with no alpha term and
// no opacity output: the entry point makes exactly the call it made before the struct existed).  target_channels: of the
// batch's targets (3 without an active background); vr_mode < 0: the entry point has no compositor (rtxn_loss).
int check_train_loss(const rtxn_train_loss* loss, int target_channels, int vr_mode, const char* who, bool* active);
// ... and its scalar in deterministic mode (loss.hip, beside l2_loss_fixed_order, same grouping and order): the sum of
// include/rtxn.h from pixels, targets and, with opacity_weight > 0, loss->opacity; with reg, the regulariser's share is added
// per ray from reg->distortion, with depth the depth term's from depth->depth and depth->target.  bg, loss, reg, depth: an ACTIVE
// struct or NULL (loss: L2).
__attribute__((visibility("hidden"))) int loss_fixed_order(const float* pixels, const float* target, int n_rays,
                                                           const rtxn_train_background* bg, const rtxn_train_loss* loss,
                                                           const rtxn_train_regularizer* reg, const rtxn_train_depth* depth, float* loss_sum,
                                                           hipStream_t stream);

// The rules of the distortion regulariser (rtxn_train_regularizer, include/rtxn.h), host only, composite_train.hip:
// RTXN_ERR_INVALID with a message naming the field, or RTXN_OK with *active = whether the regularised compositor runs at all
// (NULL, or weight 0 with no output: the entry point makes exactly the _loss call).  sample_type < 0: the entry point has none.
int check_train_regularizer(const rtxn_train_regularizer* reg, int vr_mode, int sample_type, const char* who, bool* active);

// The rules of the depth term (rtxn_train_depth, include/rtxn.h), host only, composite_train.hip: RTXN_ERR_INVALID with a message
// naming the field, or RTXN_OK with *active = whether the depth compositor runs at all (NULL, or weight 0 with no output: the
// entry point makes exactly the call of the rung below).  reg: ACTIVE or NULL, rays: NULL where the entry point has none -- an
// active term shares its t_start / t_end with both.  sample_type < 0: the entry point has none.
int check_train_depth(const rtxn_train_depth* depth, const rtxn_train_regularizer* reg, const rtxn_ray_gradients* rays, int vr_mode,
                      int sample_type, const char* who, bool* active);

// The rules of the optimizer options (rtxn_optimizer_options, include/rtxn.h), host only, optimizer.hip: RTXN_ERR_INVALID with a
// message naming the field, or RTXN_OK with *active = whether anything is switched on (NULL, or a CONSTANT schedule without
// warm-up, no decay and no guard: the entry point makes exactly the call it made before the struct existed).  need_buffers:
// an active struct must also carry lr_factor and, with skip_nonfinite, guard.
int check_optimizer_options(const rtxn_optimizer_options* opt, const char* who, bool need_buffers, bool* active);

// The rules of the loss scaler (rtxn_loss_scaler, include/rtxn.h), host only, optimizer.hip: RTXN_ERR_INVALID with a message
// naming the field.  need_buffers: the struct must also carry state and partials.
int check_loss_scaler(const rtxn_loss_scaler* scaler, const char* who, bool need_buffers);

// MurmurHash3's 32-bit finaliser: the integer hash behind RTXN_BG_RANDOM and the occupancy refresh's jitter (include/rtxn.h
// states both uses bit for bit)
__host__ __device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// RTXN_SAMPLING_JITTER_WORLD (include/rtxn.h states it bit for bit): the offset of sample s of the batch inside its stratum is a
// pure function of (seed, step, s), formed wherever a kernel forms the sample's position and never stored.  h0 is uniform over a
// launch (one scalar load and three scalar multiplies per wave); the per-sample part is one fmix32.
__device__ __forceinline__ unsigned jitter_h0(unsigned seed, const int* step) {
  const unsigned t = step ? (unsigned)*step : 0u;
  return fmix32((seed ^ 0x5BD1E995u) + 0x9E3779B9u * t);
}
__device__ __forceinline__ float jitter_u(unsigned h0, unsigned s) { return (float)(fmix32(h0 ^ s) >> 8) * 0x1p-24f; }

// The rules of a sample jitter (rtxn_sample_jitter, include/rtxn.h), host only: type 4 needs the struct, the struct needs type 4,
// and type 4's t_vals are step lengths, which RTXN_VR_COMPAT does not take (vr_mode < 0: the entry point has no compositor).
int check_sample_jitter(const char* who, int sample_type, const rtxn_sample_jitter* jitter, int vr_mode);

// The rules of the ray-gradient buffers (rtxn_ray_gradients, include/rtxn.h), host only, train.hip: a batch with a hash grid, no
// NULL among the six buffers, and t_start / t_end shared with an active regulariser (reg: ACTIVE or NULL).
int check_ray_gradients(const char* who, const rtxn_ray_gradients* rays, const rtxn_train_batch* batch, const rtxn_train_regularizer* reg);
// The rules of the pose refinement (rtxn_pose_refinement, include/rtxn.h), host only, pose.hip.  need_buffers: the struct must also
// carry its device buffers.
int check_pose_refinement(const rtxn_pose_refinement* pose, const char* who, bool need_buffers);
// The rules of the intrinsics refinement (rtxn_camera_refinement, include/rtxn.h), host only, camera_refine.hip; need_buffers as above.
int check_camera_refinement(const rtxn_camera_refinement* cameras, const char* who, bool need_buffers);

// The option structs of the training entry ladders (rtxn_train_step*, rtxn_train_gradients*), library-internal: a
// public entry point fills the pointers its signature has and leaves the rest NULL.  check_train_options replaces every
// inactive struct by NULL; own_bg / own_jitter hold a step's copies of a RANDOM background or a jitter without a counter.
struct TrainOptions {
  const rtxn_train_background* bg = nullptr;
  const rtxn_sample_jitter* jitter = nullptr;
  const rtxn_train_loss* loss = nullptr;
  const rtxn_train_regularizer* reg = nullptr;
  const rtxn_optimizer_options* opt = nullptr;
  const rtxn_loss_scaler* scaler = nullptr;
  const rtxn_weight_ema* ema = nullptr;
  const rtxn_ray_gradients* rays = nullptr;
  const rtxn_pose_refinement* pose = nullptr;
  const rtxn_camera_refinement* cameras = nullptr;
  const rtxn_train_depth* depth = nullptr;
  rtxn_train_background own_bg;
  rtxn_sample_jitter own_jitter;
};
// the rungs of both ladders, in the order they were added (the gradients ladder has no _opt and no _ema)
enum TrainRung { RUNG_PLAIN, RUNG_EX, RUNG_JITTER, RUNG_LOSS, RUNG_REG, RUNG_OPT, RUNG_SCALED, RUNG_EMA, RUNG_RAYS, RUNG_CAMERAS,
                 RUNG_DEPTH };
// The one checked path of both ladders, host only, trainer.hip: every struct's rules once, in one order, under the name the
// rung reports under (the name rule of DESIGN 5.17); then inactive structs become NULL and a step (a: its arguments, b unused)
// gets its own copies.  A gradients call passes a = NULL and its batch.
__attribute__((visibility("hidden"))) int check_train_options(TrainRung rung, bool step, const rtxn_train_step_args* a,
                                                              const rtxn_train_batch* b, TrainOptions* o);
// rtxn_train_gradients under CHECKED options (train.hip): what every rung of the gradients ladder and the one-call step run
__attribute__((visibility("hidden"))) int train_gradients(const rtxn_train_batch* b, const TrainOptions& o, rtxn_stream_t stream);

// The buffers of a training-compositor call, in the order of rtxn_volrender_l2_train's arguments
struct CompositeArgs {
  const float* network_outputs;
  const float* ray_hit;
  const int* num_hits;
  const int* indices;
  int batch_size, num_samples_per_hit;
  const float* target;
  float loss_scale;
  float* pixels;
  void* loss_gradients_half;
  float* loss_sum;
  void* radiance_gradients;
};
// The one RTXN_VR_NERF training compositor under the five rtxn_volrender_*_train entry points and rtxn_train_gradients
// (composite_train.hip): the structs' rules under `who`, then the kernel their active set selects -- nothing active: the plain
// volrender_l2_fused kernels, a background alone: volrender_l2_bg, else composite_train's, the DEV ones with scale_dev (the
// scaler's device word, read instead of c.loss_scale).  The shared checks report under the entry point that introduced the
// topmost active struct, under `who` with scale_dev.  depth (rtxn_train_depth): the DEPTH instantiations of composite_train's.
__attribute__((visibility("hidden"))) int composite_train(const char* who, const CompositeArgs& c, const rtxn_train_background* bg,
                                                          const rtxn_train_loss* loss, const rtxn_train_regularizer* reg,
                                                          const float* scale_dev, rtxn_stream_t stream, const rtxn_train_depth* depth = nullptr);
// ... and the launcher of the first two (volrender.hip, whose kernels they are); bg: ACTIVE or NULL
__attribute__((visibility("hidden"))) int l2_train(const char* who, const CompositeArgs& c, const rtxn_train_background* bg, rtxn_stream_t stream);

}  // namespace rtxn

#define RTXN_HIP(expr)                                          \
  do {                                                           \
    hipError_t e_ = (expr);                                      \
    if (e_ != hipSuccess) return ::rtxn::fail_hip(e_, #expr);    \
  } while (0)

#define RTXN_REQUIRE(cond, ...)            \
  do {                                     \
    if (!(cond)) {                         \
      ::rtxn::set_error(__VA_ARGS__);      \
      return RTXN_ERR_INVALID;             \
    }                                      \
  } while (0)

#define RTXN_LAUNCH_CHECK(name)                                   \
  do {                                                            \
    hipError_t e_ = hipGetLastError();                            \
    if (e_ != hipSuccess) return ::rtxn::fail_hip(e_, name);      \
  } while (0)

#define RTXN_DEVICE_OR_FAIL()                        \
  do {                                               \
    int rc_ = ::rtxn::require_device();              \
    if (rc_ != RTXN_OK) return rc_;                  \
  } while (0)
