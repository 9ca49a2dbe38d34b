// Launchers of the early-termination kernels (terminate.hip), sequenced per round by render.hip.  Internal to librtxn.so.
#pragma once
#include "common.h"

namespace rtxn {

// One slot's round scratch and per-ray state inside the termination workspace (rtxn_render_set_termination).
struct TermBuffers {
  int* take;          // int[max_rays]: segments the ray takes in the round being enqueued (0: dead, exhausted or never hit)
  int* off;           // int[max_rays]: exclusive scan of take = the ray's first record in the round scratch
  int* done;          // int[max_rays]: segments shaded so far; after the last round: shaded_per_ray
  int* round_total;   // int[RTXN_RENDER_MAX_ROUNDS]: segments of each round (the scan's totals)
  float4* state;      // float4[2 * max_rays]: {T, sum w r, sum w g, sum w b}, {sum w, sum w d, -, -}
  void* scan_ws;
  float* start;       // the round scratch, capacity max_segments: the records the MLP entry points read ...
  float* end;
  float* seg_view;
  void* radiance;     // ... and write: half4[max_segments * 32]
  float* seg_step;    // float[max_segments]: compact RTXN_VR_NERF only
  float* t_start;     // float[max_segments] each: RTXN_RENDER_AUX only
  float* t_end;
  long* acct;         // device long[8]: {frames, last shaded, last total, shaded, total} (rtxn_render_termination_stats)
  long* acct_host;    // pinned copy
};

struct TermOutputs {
  float* pixels;
  float* depth;       // may be NULL
  float* opacity;     // may be NULL
  float bg[3];
};

// Round 0's selection: take = min(num_stored, quota), done = 0.
int term_begin(const int* num_stored, int n_rays, int quota, const TermBuffers& b, hipStream_t s);
// Copy the records [indices + done, +take) of every ray from the slot's CSR buffers to [off, +take) of the round scratch.
int term_gather(const TermBuffers& b, const int* indices, int n_rays, long capacity, const float* start, const float* end,
                const float* seg_view, const float* t_start, const float* t_end, hipStream_t s);
// Continue every ray of the round over its take * 32 samples in the scratch, then either store its state and select
// take = min(next_quota, what is left) for the next round, or (spent, exhausted, or the last round) write its outputs.
int term_resume(const TermBuffers& b, const int* num_stored, int n_rays, int vr_mode, float u0, bool first, int next_quota,
                float t_stop, const TermOutputs& o, hipStream_t s);
// Fold the frame's round totals into the slot's 64-bit counters.
int term_account(const TermBuffers& b, int n_rounds, const int* total, int capacity, hipStream_t s);

}  // namespace rtxn
