/*
 * rtxn.h -- C ABI of librtxn.so, the MI355X (gfx950) implementation of the
 * owensgroup/rtx_nerf hot path: ray generation + ray/grid traversal, CSR
 * compaction, per-segment sampling, frequency-encoded fully-fused MLP and
 * alpha-compositing volume rendering (forward and backward).
 *
 * The reference has no FFI layer; its "operator API" is a handful of C++ free
 * functions and PODs called from main.cu.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference root).  The
 * C++ drop-in headers in include/rtxn_dropin/ (sampler/sampler.h, vol_render/vol_render.h,
 * rtx/include/params.h, loader/data_loader.h) keep the reference's own names and argument order and forward
 * to these symbols.  INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - the caller owns every buffer; the library allocates nothing per call
 *     (rtxn_mlp_create owns its packed-weight buffer until rtxn_mlp_destroy);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all
 *     work is enqueued asynchronously on it, nothing synchronises the host, so
 *     every call is hipGraph-capturable;
 *   - return value: RTXN_OK or an error code; rtxn_last_error() (host,
 *     thread-local) describes the last failure.  The reference's functions
 *     return void and print-and-continue (common/common.h:38-50).
 *   - there is no CPU fallback: without a HIP device every compute entry
 *     point fails with RTXN_ERR_HIP.
 */
#ifndef RTXN_H
#define RTXN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTXN_VERSION 100

typedef void* rtxn_stream_t;

enum rtxn_status {
  RTXN_OK = 0,
  RTXN_ERR_INVALID = 1,     /* bad argument (null pointer, negative size, unsupported width) */
  RTXN_ERR_HIP = 2,         /* a HIP runtime call or kernel launch failed */
  RTXN_ERR_UNSUPPORTED = 3, /* valid request this build does not implement */
  RTXN_ERR_IO = 4           /* loader: missing/invalid file */
};

int rtxn_version(void);
const char* rtxn_last_error(void);

/* ---- sampler/sampler.h:4-9 ------------------------------------------------ */
#define RTXN_NUM_SAMPLES_PER_SEGMENT 32
enum rtxn_sampling_type {
  RTXN_SAMPLING_REGULAR = 0,
  RTXN_SAMPLING_STRATIFIED_JITTERING = 1,
  RTXN_SAMPLING_UNIFORM = 2,
  /* not in the reference: sample i at the MIDPOINT t = (i+0.5)/32 of its sub-interval, and t_vals = the
   * sub-interval's world-space length |end-start|/32 -- the inputs RTXN_VR_NERF expects */
  RTXN_SAMPLING_MIDPOINT_WORLD = 3,
  /* not in the reference: MIDPOINT_WORLD with a fresh position inside each sub-interval per training step -- see "sample
   * jitter" below (rtxn_sample_jitter); training entry points only, and only those that take the struct */
  RTXN_SAMPLING_JITTER_WORLD = 4
};

/* ---- traversal ------------------------------------------------------------ */
/* Replaces struct Params (rtx/include/params.h:14-42), the RTXDataHolder
 * lifecycle (rtx/include/rtxFunctions.h:56-100: initContext .. buildSBT,
 * initAccelerationStructure) and optixLaunch(pipeline_ray_march, ..., W, H, 1)
 * (main.cu:506-508).  There is no acceleration structure to build: the grid of
 * make_grid (main.cu:154-174), R^3 cells over [-1,1]^3, is walked analytically;
 * `handle`, `aabb` and `num_primitives` have no counterpart. */
enum rtxn_trace_mode {
  RTXN_TRACE_COMPAT = 0, /* reference arithmetic: re-launch from each exit point (optixPrograms.cu:99-115,180-248) */
  RTXN_TRACE_DDA = 1     /* global-t 3D-DDA with hierarchical empty-space skipping; same cells, points within 1e-5 */
};

typedef struct rtxn_trace_params {
  /* rays: either a pinhole camera (look_at != NULL; params.h:17,33-34,41) ... */
  const float* look_at;      /* 16 floats, row-major 4x4, translation at [3],[7],[11] */
  float focal_length;        /* params.h:33 */
  float aspect_ratio;        /* params.h:34 */
  uint32_t width, height;    /* params.h:41 */
  /* ... or explicit rays (look_at == NULL): float3[width*height] each, d normalised */
  const float* rays_o;
  const float* rays_d;
  /* window of the launch handled by this call: rays [ray_begin, ray_begin+ray_count)
   * of the width*height launch (row-major, ray = x + y*width, optixPrograms.cu:45).
   * Outputs are indexed by the LOCAL ray number (ray - ray_begin).  This is how
   * a launch is sharded across GPUs. */
  uint32_t ray_begin, ray_count;
  /* optional interleave: local ray i maps to launch ray
   * ray_begin + (i / window_chunk) * window_stride + (i % window_chunk); 0,0 = contiguous.
   * (chunk = width, stride = n_gpus*width gives GPU g every n_gpus-th image row.) */
  uint32_t window_chunk, window_stride;
  /* grid */
  int grid_res;              /* R; cell = 2/R (main.cu:156,482) */
  const uint32_t* occupancy; /* R^3 bits, bit ((x*R+y)*R+z); NULL = dense (reference) */
  const uint32_t* occupancy_coarse; /* (R/4)^3 bits, OR of 4^3 blocks; NULL = none (from rtxn_build_occupancy_mip) */
  int mode;                  /* enum rtxn_trace_mode */
  /* outputs */
  float* ray_origins;        /* float3[ray_count]  (params.h:25), may be NULL */
  float* viewing_direction;  /* float2[ray_count]  (params.h:32), may be NULL */
  int* num_hits;             /* int[ray_count]     (params.h:31) */
  /* segment outputs; any may be NULL.  Layout: strided (reference) when
   * indices == NULL: slot = local_ray*intersection_arr_size + k
   * (optixPrograms.cu:184, main.cu:486); packed CSR when indices != NULL:
   * slot = indices[local_ray] + k (the layout main.cu:646-673 builds on the
   * host for the sampler). */
  int intersection_arr_size; /* S (params.h:19); segments beyond S are counted, not stored */
  const int* indices;
  float* start_points;       /* float3 per slot (params.h:23) */
  float* end_points;         /* float3 per slot (params.h:24) */
  float* t_start;            /* float per slot  (params.h:28) */
  float* t_end;              /* float per slot  (params.h:29) */
  int* seg_ray;              /* int per slot: local ray of the segment (packed layout; new) */
  float* seg_view;           /* float2 per slot: (theta, phi) of the segment's ray (packed layout; new) */
  long segment_capacity;     /* packed layout: slots >= capacity are not written (0 = unbounded) */
  uint8_t* seg_first;        /* byte per slot: 1 if the segment is the first of its ray (packed layout; new) */
  const uint64_t* occupancy_bricks; /* (R/4)^3 words from rtxn_build_occupancy_bricks, or NULL: the 64 fine bits of each 4^3 block
                                     * (RTXN_TRACE_DDA + occupancy_coarse only; same segments, one load per block instead of per cell) */
  const uint32_t* occupancy_super;  /* (R/16)^3 bits = rtxn_build_occupancy_mip(occupancy_coarse, R/4, .), or NULL: third level of the
                                     * empty-space hierarchy (needs occupancy_coarse, R % 16 == 0) */
  int* num_stored;           /* int[ray_count] or NULL: segments actually WRITTEN for the ray (< num_hits when
                              * intersection_arr_size / segment_capacity cut it off): the count downstream stages may read */
  int sub_rays;              /* RTXN_TRACE_DDA only; 0 or 1: one thread walks a ray.  2, 4, ... 64 (a power of two): that many adjacent lanes walk
                              * consecutive pieces of the ray's parameter range (same segments, same order, bit for bit) -- for
                              * small batches, where the launch takes as long as the longest ray's walk */
  int* sub_hits;             /* int[ray_count * sub_rays] scratch, required when sub_rays > 1: written by the counting pass,
                              * read by the write pass of the same launch geometry */
} rtxn_trace_params;

/* One launch: ray generation + grid march.  With every segment pointer NULL it
 * is the counting pass of the two-pass packed pipeline (count -> rtxn_scan_hits
 * -> write). */
int rtxn_trace_grid(const rtxn_trace_params* p, rtxn_stream_t stream);

/* Coarse occupancy mip for RTXN_TRACE_DDA: bit of coarse cell (X,Y,Z) of a
 * (R/4)^3 grid = OR over its 4^3 fine cells.  R must be a multiple of 4.
 * coarse: (R/4)^3 bits rounded up to whole uint32 words. */
int rtxn_build_occupancy_mip(const uint32_t* occupancy, int grid_res, uint32_t* coarse, rtxn_stream_t stream);

/* Brick copy of the occupancy for RTXN_TRACE_DDA: bricks[(X*Rc+Y)*Rc+Z] (Rc = R/4) holds the 64 fine bits of block
 * (X,Y,Z), bit ((x&3)<<4 | (y&3)<<2 | (z&3)). */
int rtxn_build_occupancy_bricks(const uint32_t* occupancy, int grid_res, uint64_t* bricks, rtxn_stream_t stream);

/* Occupancy maintenance (the reference only builds the dense grid once,
 * main.cu:393-399): occupancy bit of cell i = density[i] > threshold, i = (x*R+y)*R+z.
 * occupancy: ceil(R^3/32) words. */
int rtxn_occupancy_from_density(const float* density, float threshold, int grid_res, uint32_t* occupancy,
                                rtxn_stream_t stream);

/* ---- CSR compaction -------------------------------------------------------- */
/* Replaces thrust::reduce + thrust::exclusive_scan over num_hits
 * (main.cu:631-637).  indices[i] = sum_{j<i} num_hits[j]; *total = sum of all.
 * `total` is a device int: nothing is copied to the host.  workspace: at least
 * rtxn_scan_workspace_bytes(n) bytes of device scratch. */
size_t rtxn_scan_workspace_bytes(int n);
int rtxn_scan_hits(const int* num_hits, int* indices, int* total, int n, void* workspace,
                   size_t workspace_bytes, rtxn_stream_t stream);

/* ---- sampler ---------------------------------------------------------------- */
/* Replaces launchSampler (sampler/sampler.h:19-30, sampler/sampler.cu:105-131).
 * start/end: float3[P] packed; view_dirs: float2[B]; t_vals: float[P*32];
 * sampled_points: float[P*32*5] AoS (x,y,z,theta,phi); num_hits, indices:
 * int[B].  grid_res is accepted and ignored, as in the reference. */
int rtxn_sample(const float* start_points, const float* end_points, const float* view_dirs,
                float* t_vals, float* sampled_points, int batch_size, int grid_res,
                const int* num_hits, const int* indices, int sample_type, rtxn_stream_t stream);

/* ---- volume rendering --------------------------------------------------------- */
enum rtxn_volrender_mode {
  RTXN_VR_COMPAT = 0,   /* reference arithmetic, vol_render.cu:19-143, quirks included */
  RTXN_VR_NERF = 1      /* canonical NeRF quadrature: exclusive transmittance, exact analytic backward */
};

/* Replaces launch_volrender_cuda (vol_render/vol_render.h:5-13,
 * vol_render.cu:144-164).  network_inputs is accepted and ignored (the
 * reference never reads it).  network_outputs: float[P*K*4] AoS (r,g,b,sigma);
 * ray_hit: float[P*K] (the sampler's t_vals); pixels: float[B*3]. */
int rtxn_volrender_fwd(const float* network_inputs, const float* network_outputs, const int* num_hits,
                       const int* indices, const float* ray_hit, int batch_size,
                       int num_samples_per_hit, float* pixels, int mode, rtxn_stream_t stream);

/* Replaces launch_volrender_backward_cuda (vol_render/vol_render.h:15-25,
 * vol_render.cu:166-190).  loss_values is accepted and ignored.  loss_gradients:
 * half[B*3]; radiance_gradients: half[P*K*4] (stride 4, as the reference
 * writes them, vol_render.cu:108,136-139). */
int rtxn_volrender_bwd(const float* loss_values, const void* loss_gradients,
                       const float* sampled_points_radiance, const float* t_hit, const int* num_hits,
                       const int* indices, int batch_size, int num_samples_per_hit,
                       void* radiance_gradients, int mode, rtxn_stream_t stream);

/* launch_volrender_cuda + loss->evaluate (L2) + launch_volrender_backward_cuda of a training batch (main.cu:737-767) in one
 * launch, RTXN_VR_NERF arithmetic: pixels float[B*3], loss_gradients_half half[B*3] (may be NULL), *loss_sum (device float,
 * may be NULL) = sum of (pixel - target)^2 / (3B), radiance_gradients half[P*K*4].  Same values as the three entry points
 * called one after the other up to fp32 rounding of one dot product. */
int rtxn_volrender_l2_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                            int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                            void* loss_gradients_half, float* loss_sum, void* radiance_gradients, rtxn_stream_t stream);

/* The training compositor over a background (not in the reference, whose pixels are sum w_i c_i: a black background; NeRF's
 * white_bkgd / instant-ngp's random background).  rtxn_volrender_l2_train with, per ray r,
 *   pixel_r = sum w_i c_i + (1 - A) bg_r,   A = sum w_i   (the weights and A of rtxn_volrender_fwd_aux, RTXN_VR_NERF)
 * fitted by the same L2 (values (pixel - t)^2 / (3B), gradients half(loss_scale 2 (pixel - t) / (3B))) to the target t_r:
 *   target_channels 3: float[B][3], used as given;
 *   target_channels 4: float[B][4] straight (not premultiplied) RGBA, t_c = alpha rgb_c + (1 - alpha) bg_c (fp32).
 * The background bg_r of ray r (its index in the batch):
 *   RTXN_BG_CONSTANT: color[0..2];
 *   RTXN_BG_RANDOM:   fmix32(h) = MurmurHash3's finaliser (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35;
 *                     h ^= h >> 16), h0 = fmix32(seed + 0x9E3779B9u * (uint32)step), bg_c = (float)(fmix32(h0 ^ (3u r + c)) >> 8)
 *                     * 2^-24 for c = 0, 1, 2; `step` is read from the device, so a captured graph draws new backgrounds on
 *                     every replay once the counter moves.
 * The radiance gradient is the exact gradient of that pixel: written as bg + sum w_k (c_k - bg) it is the plain compositor
 * with colours c_k - bg, so dL/dc_i = g T_i a_i (unchanged) and dL/dsigma_i = d_i (T_i e^-x_i g.(c_i - bg) - sum_{k>i} w_k
 * g.(c_k - bg)).  A ray with no segments gets pixel = bg exactly and writes no radiance gradient.
 * Rules (RTXN_ERR_INVALID with a message, before any device is touched): mode NONE | CONSTANT | RANDOM; target_channels 3 | 4;
 * RANDOM needs 4 channels (a 3-channel target cannot know the background); NONE allows 3 only; no background with
 * RTXN_VR_COMPAT (its backward is not the gradient of its forward).  bg == NULL, or NONE with 3 channels: exactly the plain
 * entry point. */
enum rtxn_train_background_mode { RTXN_BG_NONE = 0, RTXN_BG_CONSTANT = 1, RTXN_BG_RANDOM = 2 };
typedef struct rtxn_train_background {
  int mode;                         /* rtxn_train_background_mode */
  float color[3];                   /* CONSTANT */
  unsigned seed;                    /* RANDOM */
  const int* step;                  /* RANDOM: DEVICE int hashed with the seed; NULL = 0 (rtxn_train_step_ex: NULL = opt.step before
                                       its increment) */
  int target_channels;              /* 3: float[n][3] targets as given; 4: float[n][4] straight RGBA, composited over this ray's
                                       background */
} rtxn_train_background;
int rtxn_volrender_l2_train_ex(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                               int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                               void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                               const rtxn_train_background* bg, rtxn_stream_t stream);

/* ---- MLP (tiny-cuda-nn surface used by main.cu) ------------------------------- */
/* Replaces tcnn::create_from_config(5, 4, config) (main.cu:35-69,325),
 * network->n_params / set_params / initialize_params (main.cu:327-349),
 * network->forward (main.cu:721) and the convertHalfToFloat glue
 * (main.cu:203-208,723-728).  Model: Composite(Frequency(n_pos_dims,
 * n_pos_freqs), Frequency(n_dir_dims, n_dir_freqs)) -> n_hidden_layers x
 * n_neurons ReLU -> 16 (n_output_dims used), fp16 weights, no biases. */
enum rtxn_activation { RTXN_ACT_NONE = 0, RTXN_ACT_SIGMOID = 1 };
enum rtxn_encoding {
  RTXN_ENC_FREQUENCY = 0, /* Composite(Frequency, Frequency) computed inside the kernels (main.cu:47-61) */
  RTXN_ENC_EXTERNAL = 1   /* the caller encodes (e.g. rtxn_hashgrid_encode); only the rtxn_mlp_train_* entry points apply */
};

typedef struct rtxn_mlp_config {
  int n_pos_dims, n_pos_freqs;   /* 3, 10 (main.cu:52-54) */
  int n_dir_dims, n_dir_freqs;   /* 2, 12 (main.cu:57-59: "n_bins" is not a Frequency key -> default 12) */
  int n_neurons;                 /* 64 or 128 (main.cu:66) */
  int n_hidden_layers;           /* >= 1 (main.cu:67) */
  int n_output_dims;             /* <= 16 (main.cu:323) */
  int output_activation;         /* enum rtxn_activation (main.cu:65) */
  int encoding;                  /* enum rtxn_encoding; 0 = the reference's Composite-Frequency */
  int n_encoded_features;        /* RTXN_ENC_EXTERNAL only: width of the pre-encoded input, multiple of 16 */
} rtxn_mlp_config;

typedef struct rtxn_mlp rtxn_mlp;
typedef struct rtxn_hashgrid rtxn_hashgrid;   /* multiresolution hash grid: rtxn_hashgrid_create, below */

int rtxn_mlp_create(const rtxn_mlp_config* cfg, rtxn_mlp** out);
int rtxn_mlp_destroy(rtxn_mlp* m);
/* number of fp16 parameters, tcnn layout: per layer a row-major [out][in]
 * matrix (first: n_neurons x enc_padded; hidden: n_neurons^2; last: 16 x
 * n_neurons), layers concatenated. */
/* The fused inference kernels run a persistent grid that fills every CU.  Work launched beside them on other streams
 * co-resides only if it fits the CU's left-over registers/LDS (this library's traversal, scan and compositor kernels do);
 * a collective library's kernels may not.  n_cus > 0 keeps that many CUs free of MLP blocks (default 0). */
int rtxn_mlp_set_reserved_cus(rtxn_mlp* m, int n_cus);
/* MFMA shape of the model's fused inference kernel: 16 = v_mfma_f32_16x16x32_f16 (every Composite-Frequency model);
 * 0 = no fused inference kernel (RTXN_ENC_EXTERNAL: use rtxn_hashmlp_forward_segments or the rtxn_mlp_train_* entry points). */
int rtxn_mlp_mfma_shape(const rtxn_mlp* m);
long rtxn_mlp_n_params(const rtxn_mlp* m);
int rtxn_mlp_padded_output_width(const rtxn_mlp* m); /* 16 (main.cu:715) */
int rtxn_mlp_encoded_width(const rtxn_mlp* m);       /* padded to a multiple of 16 */
/* Xavier-uniform init from a PCG32 stream into HOST fp32 (main.cu:344-349). */
int rtxn_mlp_initialize_params(const rtxn_mlp* m, uint64_t seed, float* host_params_fp32);
/* Point the model at device fp16 params (tcnn layout); re-packs them into the
 * MFMA fragment order the kernels read.  Call again after every update. */
int rtxn_mlp_set_params(rtxn_mlp* m, const void* params_fp16, rtxn_stream_t stream);
/* The same for a training loop's per-step update: re-packs what the rtxn_mlp_train_* entry points read and leaves the fused
 * inference kernels' copy as it was -- call rtxn_mlp_set_params before rendering with the rtxn_mlp_forward* family again. */
int rtxn_mlp_set_params_training(rtxn_mlp* m, const void* params_fp16, rtxn_stream_t stream);
/* network->forward: input float[N*5] (column-major 5xN = the sampler's AoS),
 * output half[N*16] (column-major 16xN). */
int rtxn_mlp_forward(const rtxn_mlp* m, const float* input, void* output_half, long n, rtxn_stream_t stream);
/* forward fused with the fp16->fp32 radiance glue: radiance float[N*4]. */
int rtxn_mlp_forward_radiance(const rtxn_mlp* m, const float* input, float* radiance, long n,
                              rtxn_stream_t stream);
/* Sampler (REGULAR) + encoding + MLP + glue fused: reads packed segments,
 * never materialises the 5-float samples.  seg_view: float2 per segment, the
 * (theta, phi) of its ray as written by rtxn_trace_grid (packed layout), so a
 * segment's inputs are three independent 12/12/8-byte records.
 * *total_segments is the device int written by rtxn_scan_hits; the launch is
 * sized by max_segments (capacity of the caller's buffers) and exits early
 * beyond *total_segments.
 * radiance: float[max_segments*32*4]; t_vals: float[max_segments*32] or NULL. */
int rtxn_mlp_forward_segments(const rtxn_mlp* m, const float* start_points, const float* end_points,
                              const float* seg_view, const int* total_segments, long max_segments,
                              float* radiance, float* t_vals, rtxn_stream_t stream);

/* Compact form of the two calls above for the render pipeline: the kernel stores the network's own four half outputs per
 * sample (half[N][4], 8 B instead of the 16-B float4 of convertHalfToFloat, main.cu:203-208) and no t_vals -- REGULAR
 * sampling makes them (i + 1)/32 of the sample index -- and rtxn_volrender_fwd_compact consumes exactly that.  Pixels are
 * bit-identical to rtxn_mlp_forward_segments + rtxn_volrender_fwd(RTXN_VR_COMPAT) at 40 % of the HBM traffic. */
int rtxn_mlp_forward_segments_compact(const rtxn_mlp* m, const float* start_points, const float* end_points,
                                      const float* seg_view, const int* total_segments, long max_segments,
                                      void* radiance_half4, rtxn_stream_t stream);
int rtxn_volrender_fwd_compact(const void* radiance_half4, const int* num_hits, const int* indices, int batch_size,
                               int num_samples_per_hit, float* pixels, rtxn_stream_t stream);

/* The per-ray form of the two segment entries above (64- and 128-wide Composite-Frequency models:
 * rtxn_mlp_ray_direction_bias_supported; others RTXN_ERR_UNSUPPORTED).  A segment's view direction is its ray's, so the
 * direction part of the first layer -- W values, the same for every sample of every segment of a ray -- is formed once per
 * ray and the segment kernel starts the first layer from it:
 *   rtxn_mlp_ray_direction_bias   ray_bias float[n_rays][W] (16-byte aligned) from viewing_direction float2[n_rays], as
 *                                 rtxn_trace_grid writes it; rows of rays with num_hits[ray] <= 0 are left untouched.  No host
 *                                 read: capturable.  Must be called again after rtxn_mlp_set_params.
 *   rtxn_mlp_forward_segments_rays[_compact]   as rtxn_mlp_forward_segments[_compact] with seg_ray (int per segment:
 *                                 rtxn_trace_params.seg_ray, the row of ray_bias; read clamped to n_rays - 1) and ray_bias in
 *                                 place of seg_view.
 * Outputs are bit-identical to the seg_view entries given seg_view[k] == viewing_direction[seg_ray[k]]: the same encoder, the
 * same MFMA instruction and the same k order form the same W values. */
int rtxn_mlp_ray_direction_bias_supported(const rtxn_mlp* m);
int rtxn_mlp_ray_direction_bias(const rtxn_mlp* m, const float* viewing_direction, const int* num_hits, int n_rays,
                                float* ray_bias, rtxn_stream_t stream);
int rtxn_mlp_forward_segments_rays(const rtxn_mlp* m, const float* start_points, const float* end_points, const int* seg_ray,
                                   const float* ray_bias, int n_rays, const int* total_segments, long max_segments,
                                   float* radiance, float* t_vals, rtxn_stream_t stream);
int rtxn_mlp_forward_segments_rays_compact(const rtxn_mlp* m, const float* start_points, const float* end_points,
                                           const int* seg_ray, const float* ray_bias, int n_rays, const int* total_segments,
                                           long max_segments, void* radiance_half4, rtxn_stream_t stream);
/* The same hand-over for RTXN_VR_NERF (midpoint samples, exclusive transmittance): every sample of a segment has the same
 * world-space step |end - start| / K (x density scale), so the compositor takes ONE float per segment (segment_step[P], written
 * by rtxn_hashmlp_forward_segments) instead of launch_volrender_cuda's ray_hit[P*K].  Pixels bit-identical to
 * rtxn_volrender_fwd(RTXN_VR_NERF) on the widened radiance and the expanded steps. */
int rtxn_volrender_fwd_compact_nerf(const void* radiance_half4, const float* segment_step, const int* num_hits,
                                    const int* indices, int batch_size, int num_samples_per_hit, float* pixels,
                                    rtxn_stream_t stream);

/* Colour, opacity and expected depth in one pass, with an optional background colour (not in the reference; NeRF's
 * acc_map / depth_map).  For ray r with weights w_i -- exactly those its pixel uses in vr_mode, RTXN_VR_COMPAT quirks
 * included --
 *   opacity[r] = A = sum w_i;   depth[r] = sum w_i d_i (unnormalised: divide by A for a surface depth);
 *   pixels[r]  = sum w_i c_i + (1 - A) background, the background term added per channel only where it is non-zero,
 * with d_i = t_start_j + u_i (t_end_j - t_start_j) the distance of sample i (index i in its segment j) from the ray origin:
 * u_i = i/K (REGULAR; the sampler evaluates there although its t_vals say (i+1)/K) or (i + 0.5)/K (MIDPOINT_WORLD).
 * Layouts as the three entry points above:
 *   RTXN_RADIANCE_FLOAT4: radiance float[P*K][4], ray_hit float[P*K] (t_vals / step lengths) -- rtxn_volrender_fwd;
 *   RTXN_RADIANCE_HALF4:  radiance half[P*K][4]; ray_hit NULL (RTXN_VR_COMPAT, implicit REGULAR t_vals) or segment_step
 *                         float[P] (RTXN_VR_NERF) -- rtxn_volrender_fwd_compact[_nerf].
 * t_start, t_end: float[P], the segments' entry and exit distances (rtxn_trace_params.t_start / t_end of a RTXN_TRACE_DDA
 * traversal; params.h:28-29); needed only when depth != NULL.  background: HOST float[3], or NULL = black.  depth and
 * opacity (float[B]) may each be NULL.  With a zero background the pixels are bit-identical to the entry point of the same
 * layout (same kernel choice -- pairs for even K and aligned buffers -- and the same operations).  A ray with no segments
 * gets opacity 0, depth 0 and pixel = background.  Rounding can put A a few ulp above 1 for opaque rays. */
enum rtxn_radiance_layout { RTXN_RADIANCE_FLOAT4 = 0, RTXN_RADIANCE_HALF4 = 1 };
int rtxn_volrender_fwd_aux(const void* radiance, int radiance_layout, const float* ray_hit, const int* num_hits,
                           const int* indices, const float* t_start, const float* t_end, int batch_size,
                           int num_samples_per_hit, int vr_mode, int sample_type, const float* background, float* pixels,
                           float* depth, float* opacity, rtxn_stream_t stream);

/* ---- hash-grid inference -------------------------------------------------------------------------------------------
 * launchSampler + HashGrid(position) (+) Frequency(direction) encoding + network->forward + the half outputs' glue
 * (main.cu:703-728 with the hash-grid model north_star names) as ONE kernel over packed segments: the hash-grid counterpart of
 * rtxn_mlp_forward_segments_compact.  `m` is the pre-encoded (RTXN_ENC_EXTERNAL) model a training loop trains with
 * rtxn_hashgrid_encode_segments + rtxn_mlp_train_forward_outputs; this entry point computes the SAME values as that staged
 * pair in one pass, without the half[E][S] encoding in memory.  sample_type RTXN_SAMPLING_REGULAR | RTXN_SAMPLING_MIDPOINT_WORLD.
 * radiance_half4: half[max_segments*32][4]; segment_step (may be NULL): float[max_segments], for MIDPOINT_WORLD the
 * world-space step |end - start| / 32 x t_scale of each segment -- what rtxn_volrender_fwd_compact_nerf consumes.
 * *total_segments: device int (rtxn_scan_hits' total), clamped to max_segments.
 * rtxn_hashmlp_supported: 1 if the fused kernel is built for this model / grid pair (64 wide, 1..8 hidden layers, 2 features
 * per level, an even number of levels, encoded width <= 64), else 0 (the entry point then returns RTXN_ERR_UNSUPPORTED). */
int rtxn_hashmlp_supported(const rtxn_mlp* m, const rtxn_hashgrid* g, int n_dir_freqs);
int rtxn_hashmlp_forward_segments(const rtxn_mlp* m, const rtxn_hashgrid* g, int n_dir_freqs, const void* table_fp16,
                                  const float* start_points, const float* end_points, const float* seg_view,
                                  const int* total_segments, long max_segments, int sample_type, float t_scale,
                                  void* radiance_half4, float* segment_step, rtxn_stream_t stream);

/* ---- occupancy refresh from the live model ------------------------------------------------------------------------
 * Not in the reference, which builds the dense grid once (main.cu:393-399); the update rule is instant-ngp's.  ONE call that
 * evaluates sigma at one point per cell of the R^3 grid with the fused inference kernels above, folds it into a decaying
 * running maximum, thresholds it and rewrites the whole traversal hierarchy IN PLACE -- on `stream`, without a
 * synchronisation, a host read or an allocation, so it is hipGraph-capturable and graphs that read the four buffers stay valid.
 *
 * Evaluation.  Cells (x, y, 32k .. 32k+31) form a RUN, handed to the segment kernels as one pseudo-segment whose 32 REGULAR
 * samples are the cells' sample points; NK = ceil(R/32) runs per row, global run index g = (x*R + y)*NK + k, samples of a tail
 * run beyond the grid are shaded and dropped; seg_view = (0, 0).  float32, each operation rounded on its own, in this order:
 *   h = 2.0f / (float)R;   p_x = ((float)x + 0.5f) * h - 1.0f, p_y from y, p_z from z0 = 32k;
 *   jitter != 0: step = (uint32)*step (NULL: 0), h0 = fmix32(seed + 0x9E3779B9u * step) (fmix32: see RTXN_BG_RANDOM), and for
 *                c = 0, 1, 2:  u_c = (float)(fmix32(h0 ^ (3u * (uint32)g + c)) >> 8) * 2^-24,  p_c = p_c + (u_c - 0.5f) * h
 *                -- one offset in [-0.5, 0.5) h per axis and RUN, shared by its 32 cells (a segment's samples are equally spaced on a
 *                line: a translation is the only jitter it can carry);
 *   start = p;   end = (p_x, p_y, p_z + 32.0f * h);   sample i is where the segment kernel puts it: start + (i/32)(end - start).
 * Hash models (grid != NULL) go through rtxn_hashmlp_forward_segments(RTXN_SAMPLING_REGULAR), Composite-Frequency models
 * through rtxn_mlp_forward_segments_compact; sigma is component 3 of their half[.][4] output.
 * Update, for every cell c = (x*R + y)*R + z, s = (float)sigma of its sample, NaN taken as 0:
 *   v = s * thickness_scale;   d = density[c] * decay;   density[c] = v > d ? v : d
 * (decay 0 and a zeroed density: density = max(0, v), a plain point sample).  The mean of the new density is formed in a
 * fixed order -- per run a butterfly over the 32 lanes (float), the runs' sums in double, ascending g per lane of one block,
 * then a tree -- so it does not depend on the pass size or on scheduling.
 *   thr = threshold (RTXN_OCC_ABSOLUTE) | fminf(threshold, mean) (RTXN_OCC_MIN_MEAN), read on the device;
 *   occupancy bit c = density[c] > thr (ceil(R^3/32) words, tail bits 0), then coarse = rtxn_build_occupancy_mip(occupancy),
 *   bricks = rtxn_build_occupancy_bricks(occupancy), super_mip = rtxn_build_occupancy_mip(coarse, R/4).
 * coarse and bricks must be given exactly when R % 4 == 0, super_mip exactly when R % 16 == 0 (NULL otherwise).
 * Passes: the runs are shaded runs_per_pass at a time through ONE caller-provided workspace of
 * rtxn_occupancy_refresh_workspace_bytes(grid_res, runs_per_pass) bytes (256-byte aligned; 0 with a message for bad arguments):
 * 32 B of segment records + 256 B of radiance per run of a pass, and 4 B per run of the grid.  Results are bit-identical for
 * every runs_per_pass.
 * rtxn_occupancy_refresh_supported: 1 for a Composite-Frequency model with a fused inference kernel (grid == NULL) and for a
 * hash model exactly when rtxn_hashmlp_supported; otherwise the entry returns RTXN_ERR_UNSUPPORTED.  Argument errors are
 * RTXN_ERR_INVALID with a message before any device is touched.  rtxn_mlp_set_params must have run since the last
 * rtxn_mlp_set_params_training of a frequency model (the inference kernels' rule). */
enum rtxn_occupancy_threshold_mode { RTXN_OCC_ABSOLUTE = 0, RTXN_OCC_MIN_MEAN = 1 };
typedef struct rtxn_occupancy_refresh_args {
  /* model and grid */
  const rtxn_mlp* mlp;
  const rtxn_hashgrid* grid;        /* NULL: Composite-Frequency model */
  int n_dir_freqs;                  /* hash grid only */
  const void* table_fp16;           /* hash grid only: half[rtxn_hashgrid_n_params] */
  int grid_res;                     /* R in [1, 1024] */
  /* update rule */
  float* density;                   /* float[R^3], index (x*R+y)*R+z: the running maximum, updated in place (start from zeros) */
  float decay;                      /* in [0, 1] */
  float thickness_scale;            /* sigma -> optical thickness of a cell: density scale x cell size 2/R */
  float threshold;
  int threshold_mode;               /* enum rtxn_occupancy_threshold_mode */
  /* jitter */
  int jitter;                       /* 0: cell centres */
  unsigned seed;
  const int* step;                  /* DEVICE int hashed with the seed, or NULL = 0: a captured graph draws new offsets per replay */
  /* hierarchy outputs, rewritten in place */
  uint32_t* occupancy;              /* ceil(R^3/32) words */
  uint32_t* coarse;                 /* R % 4 == 0: ceil((R/4)^3/32) words; else NULL */
  uint64_t* bricks;                 /* R % 4 == 0: (R/4)^3 words; else NULL */
  uint32_t* super_mip;              /* R % 16 == 0: ceil((R/16)^3/32) words; else NULL */
  /* optional outputs */
  int* occupied;                    /* DEVICE int or NULL: number of set fine bits */
  float* mean;                      /* DEVICE float or NULL: mean of the new density */
  /* workspace */
  void* workspace;
  size_t workspace_bytes;
  long runs_per_pass;               /* >= 1; R*R*ceil(R/32) shades the grid in one pass */
} rtxn_occupancy_refresh_args;
int rtxn_occupancy_refresh_supported(const rtxn_mlp* m, const rtxn_hashgrid* g, int n_dir_freqs);
size_t rtxn_occupancy_refresh_workspace_bytes(int grid_res, long runs_per_pass);
int rtxn_occupancy_refresh(const rtxn_occupancy_refresh_args* args, rtxn_stream_t stream);

/* ---- mesh extraction: sigma on a lattice, and its isosurface -------------------------------------------------------
 * Not in the reference.  Two entries, both on `stream` without a synchronisation, a host read, an allocation or an atomic:
 * hipGraph-capturable, and the same bytes on every run.
 *
 * rtxn_density_lattice: sigma of the model at the n_x * n_y * n_z NODES of a regular lattice over the box [lo, hi] (lo < hi, both
 * inside [-1, 1]^3, n_c in [2, 1024]), through the fused inference kernels: the occupancy refresh's evaluation without the
 * fold, the jitter and the hierarchy.  Nodes (x, y, 32k .. 32k+31) form a RUN, handed to the segment kernels as one
 * pseudo-segment whose 32 REGULAR samples are the nodes; NK = ceil(n_z/32) runs per row, run g = (x*n_y + y)*NK + k, samples
 * of a tail run beyond n_z are shaded and dropped; seg_view = (0, 0).  float32, each operation rounded on its own, in this order:
 *   h_c = (hi_c - lo_c) / (float)(n_c - 1);   P_c(i) = lo_c + (float)i * h_c;
 *   start = (P_x(x), P_y(y), P_z(32k));   end = (start_x, start_y, start_z + 32.0f * h_z);
 *   density[(x*n_y + y)*n_z + z] = s * scale,   s = (float) of the half sigma of sample z - 32k, NaN taken as 0.
 * Hash models (grid != NULL) go through rtxn_hashmlp_forward_segments(RTXN_SAMPLING_REGULAR), Composite-Frequency models
 * through rtxn_mlp_forward_segments_compact.  The runs are shaded runs_per_pass at a time through ONE caller-provided
 * workspace of rtxn_density_lattice_workspace_bytes(n, runs_per_pass) bytes (256-byte aligned; 0 with a message for bad
 * arguments): 32 B of segment records + 256 B of radiance per run of a pass.  Results are bit-identical for every
 * runs_per_pass.  Support is rtxn_occupancy_refresh_supported's rule, otherwise RTXN_ERR_UNSUPPORTED; rtxn_mlp_set_params
 * must have run since the last rtxn_mlp_set_params_training of a frequency model (the inference kernels' rule). */
typedef struct rtxn_density_lattice_args {
  const rtxn_mlp* mlp;
  const rtxn_hashgrid* grid;        /* NULL: Composite-Frequency model */
  int n_dir_freqs;                  /* hash grid only */
  const void* table_fp16;           /* hash grid only: half[rtxn_hashgrid_n_params] */
  int n[3];                         /* nodes per axis, each in [2, 1024] */
  float lo[3];                      /* lo < hi, both inside [-1, 1]^3 */
  float hi[3];
  float scale;                      /* finite; a trainer passes its density scale */
  float* density;                   /* DEVICE float[n_x*n_y*n_z], index (x*n_y + y)*n_z + z */
  void* workspace;
  size_t workspace_bytes;
  long runs_per_pass;               /* >= 1; n_x*n_y*ceil(n_z/32) shades the lattice in one pass */
} rtxn_density_lattice_args;
size_t rtxn_density_lattice_workspace_bytes(const int* n, long runs_per_pass);
int rtxn_density_lattice(const rtxn_density_lattice_args* args, rtxn_stream_t stream);

/* rtxn_isosurface: the indexed triangle mesh of {density > iso} over ANY device float lattice laid out as above (n_c in
 * [2, 1024], lo < hi finite, iso finite), by MARCHING TETRAHEDRA.  Every lattice cube is cut into the 6 tetrahedra of the Kuhn
 * triangulation along its (0,0,0)-(1,1,1) diagonal: for the axis permutation pi in lexicographic order (xyz, xzy, yxz, yzx,
 * zxy, zyx) the tet is v0 = (0,0,0), v1 = v0 + e_pi1, v2 = v1 + e_pi2, v3 = (1,1,1).  The split is translation invariant, so
 * neighbouring cubes agree on every shared face diagonal, and every tet edge leaves its lower node along one of 7 edge types,
 * d in {+x, +y, +z, +x+y, +y+z, +x+z, +x+y+z} in this order: each edge has ONE owner (node, type), its vertex is computed
 * once, and no cracks appear.
 *   Values are sanitised when read: NaN -> 0.0f, +-Inf -> +-FLT_MAX.   inside(v) = v > iso.
 *   An owned edge from node i (value a) to node i + d (value b) with inside(a) != inside(b) gets one vertex, float32, each
 *   operation rounded on its own:  t = (iso - a) / (b - a), a NaN or t < 0 -> 0, t > 1 -> 1;
 *                                  p_c = P_c(i_c) + t * ((float)d_c * h_c)      (h_c, P_c as above): finite for any input.
 *   Cases, mask bit k = inside(v_k): one vertex a alone on its side gives the triangle (a o0, a o1, a o2), the others ascending;
 *   two inside a < b and two outside c < d give (ac, ad, bd) and (ac, bd, bc); in each triangle the 2nd and 3rd entry are
 *   swapped if the normal of the edge midpoints does not point from the inside vertices' centroid to the outside vertices':
 *   triangles wind counter-clockwise seen from the side of LOWER density.  Degenerate triangles (a node equal to iso) are kept.
 *   tools/gen_tet_table.py is the definition of the table the kernel includes.
 *   Order: vertex ids in node order (x, y, z), then edge type; triangles in cube order (x, y, z), then tet, then table order.
 *   The output is a pure function of the input.
 *   normals (optional): g = the gradient of the sanitised lattice at a node -- per axis (v[i+1] - v[i-1]) / (2 h_c), at the
 *   boundary (v[1] - v[0]) / h_c and (v[n-1] - v[n-2]) / h_c -- evaluated in double at both end nodes;
 *   normal = -(g_a + t (g_b - g_a)) normalised, (0,0,0) for a zero gradient; finite for any input.
 * counts = {n_vertices, n_triangles, overflow}: the TRUE totals are always written (a total above INT_MAX is reported as
 * INT_MAX); only entries with an index below the capacity are written to the arrays, overflow = 1 if either total exceeds its
 * capacity, and triangles keep their true vertex ids in that case.  A NULL array has capacity 0: with vertices == triangles ==
 * NULL the call only counts.  Workspace: rtxn_isosurface_workspace_bytes(n) bytes (256-byte aligned; 0 with a message for bad
 * arguments): 4 B per node, 16 B per row (x, y) and 32 KB.  Argument errors are RTXN_ERR_INVALID with a message naming the field
 * before any device is touched. */
typedef struct rtxn_isosurface_args {
  const float* density;             /* DEVICE float[n_x*n_y*n_z], index (x*n_y + y)*n_z + z */
  int n[3];
  float lo[3];                      /* position of node (0, 0, 0) */
  float hi[3];                      /* position of node (n_x-1, n_y-1, n_z-1) */
  float iso;
  float* vertices;                  /* DEVICE float[max_vertices][3], or NULL */
  float* normals;                   /* DEVICE float[max_vertices][3], or NULL */
  int* triangles;                   /* DEVICE int[max_triangles][3], or NULL */
  int max_vertices;
  int max_triangles;
  int* counts;                      /* DEVICE int[3] */
  void* workspace;
  size_t workspace_bytes;
} rtxn_isosurface_args;
size_t rtxn_isosurface_workspace_bytes(const int* n);
int rtxn_isosurface(const rtxn_isosurface_args* args, rtxn_stream_t stream);

/* ---- one frame behind one call ------------------------------------------------------------------------------------
 * The per-image host sequence of the reference -- fill Params and optixLaunch (main.cu:473-508), copy every traversal
 * buffer to the host and re-pack it (:510-543, :646-673), thrust compaction (:631-637), launchSampler (:704),
 * network->forward (:721), convertHalfToFloat (:723-728), launch_volrender_cuda (:737) -- as ONE entry point that
 * enqueues   trace(count) -> scan -> trace(write packed CSR) -> sampler+encode+MLP (one kernel) -> composite
 * for a window of the width x height launch, with the segment count, the capacity clamp and the overflow flag all in
 * device memory: nothing synchronises the host, so rtxn_render_frame is hipGraph-capturable.
 *
 * rtxn_render owns no device memory of its own: the caller hands rtxn_render_create one workspace of
 * rtxn_render_workspace_bytes(cfg) bytes (256-byte aligned) in which the per-frame buffers of `n_slots` frames in flight
 * and the occupancy hierarchy (4^3 mip, bricks, 16^3 mip: rtxn_build_occupancy_*) are laid out.  Streams and events of the
 * pipelined form are created by rtxn_render_create and released by rtxn_render_destroy.
 *
 * Radiance model: `mlp` alone = a Composite-Frequency model (the fused inference kernels; rtxn_mlp_set_params must have run);
 * `mlp` + `grid` + `table_fp16` = multiresolution hash grid + Frequency(n_dir_freqs) directions feeding a pre-encoded
 * (RTXN_ENC_EXTERNAL) 64-wide model through rtxn_hashmlp_forward_segments (rtxn_mlp_set_params[_training] must have run;
 * the table is read at frame time, so a training loop may keep updating it in place). */
enum rtxn_render_flags {
  RTXN_RENDER_FLOAT4 = 1,   /* hand the compositor the reference's float4 radiance + float t_vals (convertHalfToFloat layout,
                             * 20 B/sample) instead of the network's own half4 outputs (8 B/sample); same pixels bit for bit */
  RTXN_RENDER_STABLE_INPUTS = 2,  /* rtxn_render_frame_async only: the caller promises that a frame's device inputs (the 16
                             * look_at floats, the occupancy bits) are complete BEFORE the call and stay untouched until the
                             * frame's traversal has run (pre-uploaded poses, one buffer per frame in flight).  The traversal
                             * then does not wait for the caller's stream and overlaps the previous frame's MLP kernel. */
  RTXN_RENDER_AUX = 4       /* the traversal's write pass also stores each segment's entry and exit distance (t_start,
                             * t_end: +8 B per segment of capacity in the workspace, +8 B written per segment), which the
                             * depth output of rtxn_render_frame_ex needs.  RTXN_TRACE_DDA only: the RTXN_TRACE_COMPAT walk
                             * measures its distances from each re-launched origin (as the reference's Params.t_start) */
};
typedef struct rtxn_render_config {
  const rtxn_mlp* mlp;
  const rtxn_hashgrid* grid;      /* NULL: frequency model */
  const void* table_fp16;         /* hash grid only (device) */
  int n_dir_freqs;                /* hash grid only */
  uint32_t width, height;         /* the launch (params.h:41) */
  float focal_length, aspect_ratio;
  uint32_t max_rays;              /* largest ray window a frame call will ask for (0 = width*height) */
  uint32_t window_chunk, window_stride;  /* ray interleave of this shard, as rtxn_trace_params */
  int grid_res;
  const uint32_t* occupancy;      /* R^3 bits (device) or NULL = dense; read at rtxn_render_create / rtxn_render_set_occupancy
                                   * (hierarchy build) and by every frame */
  int trace_mode;                 /* enum rtxn_trace_mode */
  int sub_rays;                   /* RTXN_TRACE_DDA: lanes per ray (rtxn_trace_params.sub_rays); 0 = 1 */
  int vr_mode;                    /* enum rtxn_volrender_mode */
  int sample_type;                /* RTXN_SAMPLING_REGULAR (frequency model: the only one) | RTXN_SAMPLING_MIDPOINT_WORLD */
  float step_scale;               /* RTXN_VR_NERF: density scale on the world-space step */
  long max_segments;              /* capacity of the packed segment buffers; a frame that needs more is truncated on the
                                   * device (never out of bounds) and reported by rtxn_render_status */
  int n_slots;                    /* frames in flight for rtxn_render_frame_async: 1..4 */
  int flags;                      /* enum rtxn_render_flags */
} rtxn_render_config;
typedef struct rtxn_render rtxn_render;

typedef struct rtxn_render_stats {
  long frames;              /* frames enqueued so far */
  long frames_checked;      /* of those, frames whose segment count has reached the host */
  long overflow_frames;     /* checked frames that needed more than max_segments (delivered truncated) */
  long max_segments_needed; /* largest segment count seen */
  long last_segments;       /* segment count of the most recently checked frame */
  long max_segments;        /* the capacity */
} rtxn_render_stats;

size_t rtxn_render_workspace_bytes(const rtxn_render_config* cfg);
int rtxn_render_create(const rtxn_render_config* cfg, void* workspace, size_t workspace_bytes, rtxn_render** out);
int rtxn_render_destroy(rtxn_render* r);
/* Rebuild the occupancy hierarchy after the bits behind cfg->occupancy changed (or point the renderer at another bitfield
 * of the same resolution).  The rebuild runs on `stream` behind whatever the caller enqueued there (the copy of the new
 * bits); `stream` first waits for pipelined traversals still in flight, and the next rtxn_render_frame_async traversal waits
 * for the rebuild.  A serial rtxn_render_frame on a DIFFERENT stream is the caller's to order. */
int rtxn_render_set_occupancy(rtxn_render* r, const uint32_t* occupancy, rtxn_stream_t stream);
/* Counting pass + scan for one pose: *segments (HOST) = packed segments the window needs.  Synchronises `stream`; for sizing
 * max_segments outside any timed region (the reference sizes by 3R slots per ray, main.cu:486). */
int rtxn_render_count_segments(rtxn_render* r, const float* look_at, uint32_t ray_begin, uint32_t ray_count, long* segments,
                               rtxn_stream_t stream);
/* One frame (or one shard of it: rays [ray_begin, ray_begin + ray_count) of the launch under the configured interleave) on
 * ONE stream, using buffer slot `slot`.  look_at: 16 floats on the DEVICE, copied into the slot first, on `stream` (so
 * ordered behind the caller's writes there).  pixels: float[ray_count][3].  Nothing synchronises; capturable.  Every slot
 * has its own buffers incl. the scan workspace: two calls on two streams with two DIFFERENT slots may run concurrently (the
 * host calls themselves one at a time). */
int rtxn_render_frame(rtxn_render* r, int slot, const float* look_at, uint32_t ray_begin, uint32_t ray_count, float* pixels,
                      rtxn_stream_t stream);
/* The same frame software-pipelined against its neighbours: traversal on an internal stream, the MLP kernel on `stream`,
 * the compositor on a second internal stream, rotating through the n_slots buffer slots, so that under the MLP kernel of
 * frame i the chip also traverses frame i+1 and composites frame i-1.  *composite_stream (may be NULL) receives the stream
 * the pixels are complete on: enqueue follow-up work on the pixels there (a gather, a copy), or call rtxn_render_drain.
 * ORDERING CONTRACT.  look_at (device) is read on the internal traversal stream.  By default that stream first waits for
 * everything the caller has enqueued on `stream` up to this call, so a pose written on `stream` (one buffer rewritten per
 * frame), new occupancy bits copied there, or a table update are all seen -- and the traversal of frame i+1 therefore starts
 * only when the MLP kernel of frame i has finished (about 3 % of an 800x800 frame).  Callers whose inputs are stable declare
 * it with RTXN_RENDER_STABLE_INPUTS (see there) and get the full overlap; then the traversal waits for `stream` only on a
 * slot's first use and after rtxn_render_set_occupancy.  Work on OTHER streams is the caller's to order.  One thread at a
 * time per renderer. */
int rtxn_render_frame_async(rtxn_render* r, const float* look_at, uint32_t ray_begin, uint32_t ray_count, float* pixels,
                            rtxn_stream_t stream, rtxn_stream_t* composite_stream);
/* As rtxn_render_frame_async with the pose in HOST memory, where the reference keeps it (main.cu:481-501 fills Params from a
 * host look_at): the 16 floats are copied into pinned staging owned by the slot before the call returns (the caller may
 * reuse its array at once) and uploaded on the traversal stream, so the pipeline overlaps fully without any promise. */
int rtxn_render_frame_async_host(rtxn_render* r, const float* look_at_host, uint32_t ray_begin, uint32_t ray_count,
                                 float* pixels, rtxn_stream_t stream, rtxn_stream_t* composite_stream);
/* What a frame call writes beyond the pixels (rtxn_volrender_fwd_aux has the definitions).  pixels: float[ray_count][3]
 * (required); depth, opacity: float[ray_count], each may be NULL -- depth needs a renderer created with RTXN_RENDER_AUX,
 * opacity and the background work on every renderer.  background: added as (1 - opacity) x background per channel where it
 * is non-zero; all zero = the pixels of rtxn_render_frame bit for bit.  The background travels as a kernel argument: a
 * captured graph keeps the background it was captured with. */
typedef struct rtxn_render_outputs {
  float* pixels;
  float* depth;
  float* opacity;
  float background[3];
} rtxn_render_outputs;
/* rtxn_render_frame and rtxn_render_frame_async[_host] with the outputs above: same stages, same streams, same ordering
 * contract, and every output complete where the pixels are (on `stream`, resp. on *composite_stream).  pose_on_host != 0:
 * look_at is a HOST array, as rtxn_render_frame_async_host.  rtxn_render_frame_ex is capturable like rtxn_render_frame;
 * the async form, like its counterparts, is not. */
int rtxn_render_frame_ex(rtxn_render* r, int slot, const float* look_at, uint32_t ray_begin, uint32_t ray_count,
                         const rtxn_render_outputs* outputs, rtxn_stream_t stream);
int rtxn_render_frame_async_ex(rtxn_render* r, const float* look_at, int pose_on_host, uint32_t ray_begin, uint32_t ray_count,
                               const rtxn_render_outputs* outputs, rtxn_stream_t stream, rtxn_stream_t* composite_stream);
/* Make `stream` wait for everything rtxn_render_frame_async has enqueued on the internal streams. */
int rtxn_render_drain(rtxn_render* r, rtxn_stream_t stream);
/* Overflow report without polling the device.  Every frame updates four per-slot counters ON THE DEVICE (segments of the
 * frame, frames, frames over capacity, largest count) and copies them to pinned host memory (16 bytes, async); the counters
 * are cumulative, so frames replayed from a captured hipGraph are counted once per replay.  This call folds in the copies
 * that have arrived (wait != 0: synchronises the device first, so every enqueued or replayed frame is seen). */
int rtxn_render_status(rtxn_render* r, int wait, rtxn_render_stats* out);
/* Device buffers of a slot for inspection (tests, profiling tools); any out pointer may be NULL.  num_stored = segments
 * actually written per ray; t_vals: RTXN_RENDER_FLOAT4 only, segment_step: compact RTXN_VR_NERF only (else NULL). */
int rtxn_render_slot_buffers(rtxn_render* r, int slot, const int** num_hits, const int** num_stored, const int** indices,
                             const int** total_segments, const float** start_points, const float** end_points,
                             const float** seg_view, const void** radiance, const float** t_vals, const float** segment_step,
                             const float** viewing_direction);
/* Per-ray shading of the frequency model's frame (rtxn_mlp_forward_segments_rays*): with a RAY WORKSPACE set, every frame entry
 * -- serial, pipelined, captured -- also has the write pass store each segment's slot-local ray (rtxn_trace_params.seg_ray),
 * forms layer 0's direction product once per ray with a hit right behind the counting pass, on the stream the traversal runs
 * on (rtxn_mlp_ray_direction_bias), and shades from that table: the same radiance and pixels bit for bit, 1.6 % fewer MFMAs
 * and 6 % fewer LDS reads in the kernel that is the frame.  The table is per slot and lives as long as the slot's segments.
 * The workspace is the caller's (256-byte aligned), per slot int[max_segments] + float[max_rays][n_neurons] -- dense over the
 * rays, 512 B per ray of a 128-wide model, of which only rows of rays with a hit are written or read;
 * rtxn_render_ray_workspace_bytes is 0 (and says nothing) for models without per-ray kernels: hash-grid and 256-wide ones.
 * rtxn_render_set_ray_workspace synchronises the device; workspace == NULL turns per-ray shading off again.  The main
 * workspace, the termination rounds (which gather seg_view) and the public segment entries are unchanged.  A pipelined frame
 * that follows rtxn_mlp_set_params* has its traversal wait for `stream` once: the table is built from the packed weights.
 * rtxn_render_ray_buffers: the slot's two buffers for inspection, NULL without a ray workspace. */
size_t rtxn_render_ray_workspace_bytes(const rtxn_render_config* cfg);
int rtxn_render_set_ray_workspace(rtxn_render* r, void* workspace, size_t workspace_bytes);
int rtxn_render_ray_buffers(rtxn_render* r, int slot, const int** seg_ray, const float** ray_bias);

/* ---- early termination of the frame entry --------------------------------------------------------------------------
 * Not in the reference, whose loop shades every sample of every ray (main.cu:703-737).  With a termination set,
 * rtxn_render_frame and rtxn_render_frame_ex shade a frame's rays front to back in n_rounds ROUNDS and stop shading a ray
 * once its transmittance is spent.  Round k < n_rounds - 1 takes the next first_round_segments * 2^k segments of every ray
 * still alive, round n_rounds - 1 all that remain; a ray enters round 0 if it has a stored segment (num_stored, so a frame
 * over capacity is truncated exactly as before), and after a round's samples are composited it stays alive iff it has
 * segments left and T <= t_stop = -logf(min_transmittance) (host, once), T being the optical depth its compositing mode
 * has accumulated over the samples shaded so far (RTXN_VR_COMPAT: the running T of vol_render.cu:60, un-reset t_prev
 * included; RTXN_VR_NERF: sum sigma delta).  The outputs are those of rtxn_volrender_fwd_aux over the shaded prefix of each
 * ray, nothing renormalised: opacity = sum w_i, depth = sum w_i d_i, pixels = sum w_i c_i + (1 - opacity) background.
 * Both modes give w_i <= exp(-T_{i-1}) - exp(-T_i), so what is left out sums to at most exp(-T) < min_transmittance:
 * against the unterminated frame, opacity and every pixel channel (colours in [0,1]) move by at most min_transmittance,
 * depth by at most min_transmittance x the largest sample distance.
 * The caller owns a SECOND workspace of rtxn_render_termination_workspace_bytes() bytes (256-byte aligned; 0 with a message
 * for bad arguments): per slot one round's packed segment records and radiance at capacity max_segments, and 44 B per ray
 * of round counts, offsets and carried state.  Every count stays on the device, so terminated frames are capturable like
 * plain ones.  Supported: the compact hand-overs (not RTXN_RENDER_FLOAT4: RTXN_ERR_UNSUPPORTED).  While a termination is
 * set the rtxn_render_frame_async* entries return RTXN_ERR_UNSUPPORTED.  rtxn_render_set_termination validates its
 * arguments before any device is touched, synchronises the device (a set-up call) and resets the termination counters;
 * term == NULL switches termination off (workspace ignored): frames are then the plain ones, bit for bit. */
#define RTXN_RENDER_MAX_ROUNDS 8
typedef struct rtxn_render_termination {
  float min_transmittance;     /* a ray is not shaded further once exp(-T) < this at a round boundary; inside (0, 1) */
  int first_round_segments;    /* segments per living ray in round 0; >= 1 */
  int n_rounds;                /* 1..RTXN_RENDER_MAX_ROUNDS; 1 shades everything in one round */
} rtxn_render_termination;
size_t rtxn_render_termination_workspace_bytes(const rtxn_render_config* cfg, const rtxn_render_termination* term);
int rtxn_render_set_termination(rtxn_render* r, const rtxn_render_termination* term, void* workspace, size_t bytes);
/* Segment counts of terminated frames.  Each such frame adds to 64-bit per-slot counters ON THE DEVICE and copies them to
 * pinned host memory (async), so a frame replayed from a captured hipGraph counts once per replay.  total = segments the
 * frame stored (what the plain frame shades), shaded = segments the rounds shaded; last_* quote the slot used most recently.
 * wait != 0 synchronises the device first; wait == 0 reports what has arrived. */
typedef struct rtxn_render_termination_stats {
  long frames;
  long last_shaded_segments;
  long last_total_segments;
  long shaded_segments;
  long total_segments;
} rtxn_render_termination_stats;
int rtxn_render_termination_status(rtxn_render* r, int wait, rtxn_render_termination_stats* out);
/* shaded_per_ray: DEVICE int[max_rays] of slot `slot`, the segments of each ray the last terminated frame shaded (tests,
 * tools).  RTXN_ERR_INVALID before the first rtxn_render_set_termination. */
int rtxn_render_termination_buffers(rtxn_render* r, int slot, const int** shaded_per_ray);

/* ---- training path (tiny-cuda-nn surface of main.cu:721-787) ------------------------ */
/* Per-sample training tensors are FEATURE-MAJOR fp16: X[feature][S_pad] with
 * S_pad = rtxn_padded_samples(S) (S rounded up to 256), padding columns zero. */
long rtxn_padded_samples(long n_samples);

/* Encoders: input float[S][5] (x,y,z in [-1,1]; theta,phi) -> encT half[E][S_pad]. */
int rtxn_encode_frequency(const rtxn_mlp* m, const float* input, void* encT, long n_samples, rtxn_stream_t stream);

/* Multiresolution hash grid (Mueller et al. 2022, tcnn "HashGrid") for the position, composed
 * with Frequency(n_dir_freqs) for the view direction; width padded to 16 with ones. */
typedef struct rtxn_hashgrid_config {
  int n_levels;            /* <= 16 */
  int n_features;          /* per level: 1, 2, 4 or 8 */
  int log2_hashmap_size;   /* table entries per level = min(dense level size, 2^this) */
  int base_resolution;
  float per_level_scale;
} rtxn_hashgrid_config;
int rtxn_hashgrid_create(const rtxn_hashgrid_config* cfg, rtxn_hashgrid** out);
int rtxn_hashgrid_destroy(rtxn_hashgrid* g);
long rtxn_hashgrid_n_params(const rtxn_hashgrid* g);                 /* fp16 table entries */
int rtxn_hashgrid_encoded_width(const rtxn_hashgrid* g, int n_dir_freqs);
/* Table layout for callers that treat levels differently (the data-parallel gradient exchange): offset of a level in
 * PARAMETERS (entries x n_features; level == n_levels gives the total), and whether the level is hashed (its dense size
 * exceeds 2^log2_hashmap_size) or stored densely.  Dense levels come first. */
long rtxn_hashgrid_level_offset(const rtxn_hashgrid* g, int level);
int rtxn_hashgrid_level_is_hashed(const rtxn_hashgrid* g, int level);
int rtxn_hashgrid_encode(const rtxn_hashgrid* g, int n_dir_freqs, const void* table_fp16, const float* input,
                         void* encT, long n_samples, rtxn_stream_t stream);
/* dtable (fp32, table layout) += scatter of dencT; the caller zeroes dtable per step. */
int rtxn_hashgrid_backward(const rtxn_hashgrid* g, const float* input, const void* dencT, long n_samples,
                           float* dtable, rtxn_stream_t stream);

/* launchSampler folded into its consumers: the encoders and the hash-grid scatter take the packed SEGMENTS (start/end float3
 * per segment, seg_view float2 per segment as rtxn_trace_grid writes them) and form sample (segment g, i) themselves exactly
 * as rtxn_sample would -- sample_type RTXN_SAMPLING_REGULAR or RTXN_SAMPLING_MIDPOINT_WORLD (the deterministic modes) -- so the
 * 20-byte samples (sampler/sampler.h:19-30, `d_sampled_points`) never exist in memory.  n_samples = 32 n_segments.
 * t_vals (may be NULL): the sampler's t_vals, float[n_segments * 32], times t_scale (MIDPOINT_WORLD: world step x density
 * scale; REGULAR: (i + 1)/32, t_scale ignored).  backward_segments: dtable_hashed_half NULL = all levels fp32
 * (rtxn_hashgrid_backward), else the mixed form (rtxn_hashgrid_backward_mixed). */
int rtxn_encode_frequency_segments(const rtxn_mlp* m, const float* start_points, const float* end_points, const float* seg_view,
                                   long n_segments, int sample_type, float t_scale, void* encT, float* t_vals,
                                   rtxn_stream_t stream);
int rtxn_hashgrid_encode_segments(const rtxn_hashgrid* g, int n_dir_freqs, const void* table_fp16, const float* start_points,
                                  const float* end_points, const float* seg_view, long n_segments, int sample_type,
                                  float t_scale, void* encT, float* t_vals, rtxn_stream_t stream);
int rtxn_hashgrid_backward_segments(const rtxn_hashgrid* g, const float* start_points, const float* end_points, long n_segments,
                                    int sample_type, const void* dencT, float* dtable, void* dtable_hashed_half,
                                    rtxn_stream_t stream);

/* As rtxn_hashgrid_backward, with the HASHED levels' gradient accumulated in fp16 (n_features == 2: one
 * global_atomic_pk_add_f16 per corner instead of two fp32 atomics -- the scatter is bound by atomic instructions -- and what
 * tiny-cuda-nn does: its grid gradient is __half2).  dtable: fp32, whole-table layout, receives the densely stored levels;
 * dtable_hashed_half: fp16, the parameters from rtxn_hashgrid_level_offset(first hashed level) on.  Both accumulated into. */
int rtxn_hashgrid_backward_mixed(const rtxn_hashgrid* g, const float* input, const void* dencT, long n_samples,
                                 float* dtable, void* dtable_hashed_half, rtxn_stream_t stream);

/* network->forward with saved activations (main.cu:721).  workspace: at least
 * rtxn_mlp_train_workspace_bytes(m, S) bytes, shared with the backward call.
 * output_half: half[S][16]; radiance: float[S][4] or NULL (the glue of main.cu:723-728). */
size_t rtxn_mlp_train_workspace_bytes(const rtxn_mlp* m, long n_samples);
int rtxn_mlp_train_forward(const rtxn_mlp* m, const void* encT, long n_samples, void* workspace,
                           void* output_half, float* radiance, rtxn_stream_t stream);
/* network->backward (main.cu:781).  dout_half4: half[S][4], the layout
 * launch_volrender_backward_cuda writes (stride 4; output rows 4..15 carry no gradient).
 * dparams: float[n_params] in the tcnn parameter layout, ACCUMULATED into (zero it per step);
 * dencT: half[E][S_pad] gradient w.r.t. the encoded input, or NULL. */
int rtxn_mlp_train_backward(const rtxn_mlp* m, const void* encT, const void* output_half, const void* dout_half4,
                            long n_samples, void* workspace, float* dparams, void* dencT, rtxn_stream_t stream);

/* Recompute path for models whose whole gradient fits on the chip (64 wide, <= 4 hidden layers, encoded width <= 64:
 * BASELINE configs[2]).  network->forward (main.cu:721) WITHOUT saved activations, and network->backward (main.cu:781) as ONE
 * kernel that rebuilds the activations in registers from encT, runs the dgrad chain and accumulates every layer's weight
 * gradient on the chip (LDS-transposed operands, one pass of atomics per wave): no per-sample, per-layer tensor touches HBM
 * and no workspace is needed.  Same results as rtxn_mlp_train_forward + rtxn_mlp_train_backward up to fp32 summation order.
 * rtxn_mlp_train_recompute_supported: 1 if this model can use the pair, else 0 (backward_recompute then returns
 * RTXN_ERR_UNSUPPORTED; forward_outputs works for every trainable width). */
int rtxn_mlp_train_recompute_supported(const rtxn_mlp* m);
int rtxn_mlp_train_forward_outputs(const rtxn_mlp* m, const void* encT, long n_samples, void* output_half, float* radiance,
                                   rtxn_stream_t stream);
int rtxn_mlp_train_backward_recompute(const rtxn_mlp* m, const void* encT, const void* output_half, const void* dout_half4,
                                      long n_samples, float* dparams, void* dencT, rtxn_stream_t stream);

/* Lean path for the reference's own model (128 wide, 8 hidden layers, 112 encoded features: main.cu:35-69), where the whole
 * gradient does not fit on the chip.  The saved-activation pair above moves 8.8 KB per sample through device memory (2 KB of
 * activations out of the forward, 2 KB of dZ out of the backward chain, both back into the weight-gradient GEMM) and needs a
 * workspace of 4.3 KB per sample -- 40 GB at the reference's batch (main.cu:186).  Here the forward keeps only the 16-byte
 * sign masks per sample and layer (all the backward chain needs of the activations), the chain writes dZ as before, and the
 * weight gradient RECOMPUTES the activations from the encoded input in three passes (layers 0-2, 3-5, 6-7 + output) with the
 * gradients accumulated on chip: 5.4 KB moved (4.4 with the _segments pair below, which needs no encT) and 2.2 KB of workspace per sample.  Same results as the pair above up to the
 * summation order of the fp32 atomics.
 *   rtxn_mlp_train_lean_supported: 1 if the model has this path;
 *   workspace_lean: rtxn_mlp_train_lean_workspace_bytes(m, n_samples) bytes, written by _forward_lean, read by _backward_lean;
 *   live_ws (may be NULL): as rtxn_mlp_train_backward_live -- only the listed segments are visited. */
int rtxn_mlp_train_lean_supported(const rtxn_mlp* m);
size_t rtxn_mlp_train_lean_workspace_bytes(const rtxn_mlp* m, long n_samples);
int rtxn_mlp_train_forward_lean(const rtxn_mlp* m, const void* encT, long n_samples, void* workspace_lean, void* output_half,
                                float* radiance, rtxn_stream_t stream);
/* The same forward with the encoder folded in (the reference's model only: Composite-Frequency with 3 x 10 position and 2 x 12
 * direction frequencies, main.cu:35-69; _fused_supported says so): the samples are formed from the packed segments as
 * rtxn_encode_frequency_segments forms them and encoded straight into the first layer's operands -- bit for bit the values
 * _forward_lean reads out of encT; t_vals (may be NULL) as rtxn_encode_frequency_segments writes them.  _backward_lean_segments is the
 * matching backward: its weight gradient recomputes the encoding with the activations, a column tile's segment constants through
 * the scalar cache.  With the pair no encT exists at all (main.cu:721,781 are tcnn calls that encode and multiply in one):
 * 3.6 instead of 4.8 KB per sample through device memory (the pair also forms the last hidden layer's dZ on chip), and no encoder launch. */
int rtxn_mlp_train_forward_lean_fused_supported(const rtxn_mlp* m);
int rtxn_mlp_train_forward_lean_segments(const rtxn_mlp* m, const float* start_points, const float* end_points, const float* seg_view,
                                         long n_segments, int sample_type, float t_scale, float* t_vals, void* workspace_lean,
                                         void* output_half, float* radiance, rtxn_stream_t stream);
int rtxn_mlp_train_backward_lean_segments(const rtxn_mlp* m, const float* start_points, const float* end_points, const float* seg_view,
                                          long n_segments, int sample_type, const void* output_half, const void* dout_half4,
                                          void* workspace_lean, const void* live_ws, float* dparams, rtxn_stream_t stream);
int rtxn_mlp_train_backward_lean(const rtxn_mlp* m, const void* encT, const void* output_half, const void* dout_half4,
                                 long n_samples, void* workspace_lean, const void* live_ws, float* dparams, rtxn_stream_t stream);

/* loss->evaluate (tcnn "L2", main.cu:36-38,759): values[i] = d^2/n, grads[i] = loss_scale*2d/n (half),
 * *loss_sum (device float) = sum of values.  values/grads/loss_sum may each be NULL. */
int rtxn_l2_loss(const float* pred, const float* target, long n, float loss_scale, float* values, void* grads_half,
                 float* loss_sum, rtxn_stream_t stream);
/* optimizer->step (tcnn "Adam", main.cu:40-46,787): fp32 master weights + fp16 copy, fp32 gradients. */
int rtxn_adam_step(long n, float* master, void* params_fp16, const float* grads, float* m, float* v, int step,
                   float lr, float beta1, float beta2, float eps, float loss_scale, rtxn_stream_t stream);

/* rtxn_adam_step with the gradient in fp16 (the hashed levels' table gradient, rtxn_hashgrid_backward_mixed). */
int rtxn_adam_step_half_grads(long n, float* master, void* params_fp16, const void* grads_fp16, float* m, float* v, int step,
                              float lr, float beta1, float beta2, float eps, float loss_scale, rtxn_stream_t stream);

/* The two Adam entry points for a step that is replayed as a hipGraph: the bias-corrected rate lr*sqrt(1-beta2^t)/(1-beta1^t)
 * depends on the step number, which must not be baked into the captured launch, so it is read from DEVICE memory
 * (*effective_lr) -- the caller refreshes it before every replay (e.g. an H2D copy node from pinned memory holding
 * rtxn_adam_effective_lr(lr, beta1, beta2, t), which is exactly the value rtxn_adam_step computes on the host).
 * Accuracy of the rate (this function: powf; rtxn_optimizer_rate: the powers in double, rounded to float once): the rounded
 * power stands against 1 - beta^t, so the relative error against float64 is bounded by 5.5 roundings plus half an ulp (powf:
 * one) of beta2^t over 2 (1 - beta2^t) and of beta1^t over 1 - beta1^t -- 1.6e-5 at t = 1 for the default betas, 1.5e-4 at
 * beta2 = 0.9999, below 1e-4 for beta2 <= 0.9998; measured within it (tests/_adam_float64.py: rho_dense).
 * grad_flags: RTXN_ADAM_GRADS_FP16: `grads` is half[n] (as rtxn_adam_step_half_grads), else float[n];
 * RTXN_ADAM_ZERO_GRADS: the gradient is cleared as it is consumed, so the next step accumulates into zeros without a
 * separate fill pass over the (tens of MB of) table gradient. */
enum rtxn_adam_grad_flags { RTXN_ADAM_GRADS_FP16 = 1, RTXN_ADAM_ZERO_GRADS = 2 };
float rtxn_adam_effective_lr(float lr, float beta1, float beta2, int step);
int rtxn_adam_step_captured(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                            const float* effective_lr, float beta1, float beta2, float eps, float loss_scale,
                            rtxn_stream_t stream);
/* tiny-cuda-nn's Adam for its "non-matrix" parameters, i.e. the hash table (optimizers/adam.h, adam_step -- [upstream], the
 * reference's optimizer, main.cu:36-46,787): an entry whose gradient is EXACTLY zero is skipped (moments and weight unchanged),
 * and the bias correction lr*sqrt(1-beta2^t)/(1-beta1^t) uses the entry's own update count t = ++param_steps[i] (uint32[n],
 * zero-initialised, part of the optimizer state).  No step number in the arguments: the call is capturable as it is.
 * Accuracy of that rate: beta^t is one exp2 instruction of t * (float)log2(beta), so its relative error against float64 is
 * bounded by one ulp of beta^t over 1 - beta^t (halved under the root for beta2) plus 5.5 roundings, largest at t = 1: 4.1e-6
 * at betas (0.9, 0.99), 3.1e-5 at the default (0.9, 0.999), 3.0e-4 at (0.9, 0.9999) -- below 1e-4 for beta2 <= 0.9996; measured
 * on the MI355X: 5.6e-7, 3.3e-6 and 5.0e-5 at most (tests/_adam_float64.py: rho_sparse; tests/test_gpu_adam_float64.py).
 * grad_flags as rtxn_adam_step_captured.  HBM: the gradient everywhere, the 18 B of state per parameter only where it is
 * non-zero (a batch touches 0.2 .. 25 % of a hashed level). */
int rtxn_adam_step_sparse(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                          unsigned* param_steps, float lr, float beta1, float beta2, float eps, float loss_scale,
                          rtxn_stream_t stream);

/* ---- deterministic training (debugging, tight comparisons) ------------------------------------------------------------
 * By default every gradient sum that crosses workgroups is a float atomic (the weight-gradient kernels' final flush; the hash
 * scatter, packed fp16 on the hashed levels as tiny-cuda-nn does): two runs of one step differ in the last bits, which Adam's
 * 1/sqrt(v) turns into +-lr on entries whose gradient is noise around zero.  With shadows registered here those sums are
 * accumulated in 64-bit fixed point (value x 2^40, integer atomics: order-independent) and folded into the gradient buffers
 * once per call, so identical inputs give identical bits, run after run and across data-parallel ranks.
 *   mlp_shadow:   rtxn_deterministic_workspace_bytes(rtxn_mlp_n_params) bytes, zeroed once by the caller, or NULL;
 *   table_shadow: rtxn_deterministic_workspace_bytes(rtxn_hashgrid_n_params) bytes, zeroed once, or NULL (no hash grid).
 * Process-wide and read when a backward / scatter entry point is CALLED (so: baked into a captured graph); (NULL, NULL)
 * restores the default.  The folds leave the shadows zero.  Costs: 8-byte atomics in the scatter (about 2x its time) and one
 * sweep over each shadow per call.  The loss scalar of rtxn_volrender_l2_train[_ex] (and of rtxn_train_gradients* /
 * rtxn_train_step*, which call them) is covered too: with a shadow registered it is summed behind the compositor in a fixed
 * order (groups of four rays, ascending) from the pixels and targets, one small launch more, instead of by the compositor's
 * float atomics (one per block of four rays, or one per ray for odd K or misaligned buffers).  Not covered: rtxn_l2_loss's sum (the three-launch compositor path; a float atomic, it feeds nothing back).
 * Range: a single contribution that is NaN, +-Inf or of magnitude >= 2^22 marks its element (a bitmap behind the sums, part of
 * the workspace size) and the fold writes a quiet NaN there -- as the float atomics would propagate NaN / Inf.  What is NOT
 * caught: in-range contributions whose running sum passes +-2^23 wrap around in the 64-bit integer and fold to a finite, wrong
 * value; keep |gradient element| < 2^23 (loss scale) in this mode. */
size_t rtxn_deterministic_workspace_bytes(long n_params);
int rtxn_set_deterministic_workspace(void* mlp_shadow, void* table_shadow);

/* ---- one training batch without a host round trip ------------------------------------------------------------------
 * The body of the reference's training loop between the traversal and the optimizer (main.cu:703-781: launchSampler ->
 * network->forward -> launch_volrender_cuda -> loss->evaluate -> launch_volrender_backward_cuda -> network->backward) as
 * ONE call whose kernels take the batch's segment count from the device (`total_segments`, as rtxn_scan_hits leaves it;
 * clamped to segment_capacity), where the reference -- and the per-stage entry points above -- need it on the host
 * (main.cu:632 synchronises for it).  Nothing in the call synchronises or allocates, so traversal + this call + the
 * optimizer can be captured into a hipGraph and replayed.  Same kernels and results as the per-stage sequence
 *   rtxn_hashgrid_encode_segments | rtxn_encode_frequency_segments -> rtxn_mlp_train_forward[_outputs] ->
 *   rtxn_volrender_l2_train (RTXN_VR_NERF) | rtxn_volrender_fwd + rtxn_l2_loss + rtxn_volrender_bwd (RTXN_VR_COMPAT) ->
 *   rtxn_mlp_train_backward[_recompute] -> rtxn_hashgrid_backward_segments
 * with one difference in layout only: the feature-major workspaces use the row stride of the CAPACITY,
 * rtxn_padded_samples(32 * segment_capacity), every step.  All buffers are the caller's, sized for segment_capacity
 * segments; the gradient outputs are ACCUMULATED into (zero them first). */
typedef struct rtxn_train_batch {
  const rtxn_mlp* mlp;
  const rtxn_hashgrid* grid;        /* NULL: the model's own Composite-Frequency encoding */
  int n_dir_freqs;                  /* hash grid only: Frequency(n) on the two direction dimensions */
  const void* table_fp16;           /* hash grid only: half[rtxn_hashgrid_n_params] */
  /* the batch's packed segments (rtxn_trace_grid write pass) */
  const float* start_points;        /* float[capacity][3] */
  const float* end_points;          /* float[capacity][3] */
  const float* seg_view;            /* float[capacity][2] */
  const int* num_stored;            /* int[n_rays]: segments per ray actually stored */
  const int* indices;               /* int[n_rays]: first segment of each ray */
  const int* total_segments;        /* DEVICE int: segments of this batch (rtxn_scan_hits' total) */
  long segment_capacity;
  int n_rays;
  int sample_type;                  /* RTXN_SAMPLING_REGULAR | RTXN_SAMPLING_MIDPOINT_WORLD (| RTXN_SAMPLING_JITTER_WORLD: the _jitter forms) */
  float t_scale;                    /* MIDPOINT_WORLD: factor on the step lengths written to t_vals */
  int vr_mode;                      /* RTXN_VR_COMPAT | RTXN_VR_NERF */
  const float* targets;             /* float[n_rays][3] */
  float loss_scale;
  /* workspaces */
  void* encT;                       /* half[E][Sp], Sp = rtxn_padded_samples(32 * capacity) */
  void* dencT;                      /* half[E][Sp]; hash grid only */
  void* workspace;                  /* rtxn_mlp_train_workspace_bytes(mlp, 32 * capacity), or NULL: recompute path
                                       (rtxn_mlp_train_recompute_supported) */
  void* output_half;                /* half[32 * capacity][16] */
  float* radiance;                  /* float[32 * capacity][4] */
  float* t_vals;                    /* float[32 * capacity] */
  void* radiance_gradients;         /* half[32 * capacity][4] */
  /* outputs */
  float* pixels;                    /* float[n_rays][3] */
  void* loss_gradients_half;        /* half[n_rays][3] */
  float* loss_sum;                  /* device float (may be NULL): mean squared error of the batch */
  float* dparams;                   /* float[rtxn_mlp_n_params], accumulated into */
  float* dtable;                    /* hash grid: float[n_params], accumulated into */
  void* dtable_hashed_half;         /* hash grid, optional: as rtxn_hashgrid_backward_segments */
  void* live_ws;                    /* optional: rtxn_live_segments_workspace_bytes(capacity); the backward then
                                       visits only the segments that carry a loss gradient (rtxn_live_segments) */
  int skip_table_backward;          /* hash grid: != 0 stops after network->backward (dparams and dencT complete): the caller
                                       runs rtxn_hashgrid_backward_segments[_live] itself -- data parallel: after handing the MLP
                                       gradient to its all-reduce, which then runs beside the scatter */
  int workspace_lean;               /* != 0: `workspace` is a LEAN workspace (rtxn_mlp_train_lean_workspace_bytes; models with
                                       rtxn_mlp_train_lean_supported): no activations are saved, the weight gradient recomputes them */
} rtxn_train_batch;
int rtxn_train_gradients(const rtxn_train_batch* batch, rtxn_stream_t stream);
/* rtxn_train_gradients over a background (rtxn_volrender_l2_train_ex): batch->targets are float[n_rays][bg->target_channels];
 * RTXN_VR_NERF only.  bg == NULL or NONE with 3 channels: exactly rtxn_train_gradients. */
int rtxn_train_gradients_ex(const rtxn_train_batch* batch, const rtxn_train_background* bg, rtxn_stream_t stream);

/* ---- one optimisation step as one call -------------------------------------------------------------------------------
 * The body of the reference's training loop for one batch of rays (main.cu:619-805): traversal (count -> scan -> write, the
 * packed layout of main.cu:646-673 written by the device) -> rtxn_train_gradients -> optimizer->step -> training-weight
 * re-pack, enqueued on ONE stream with no host round trip (the reference synchronises for the segment count, main.cu:632, and
 * re-packs the segments on the host).  Nothing in it allocates or synchronises: captured once into a hipGraph it is replayed per
 * step with only the ray and target buffers refreshed.  The optimizer is tiny-cuda-nn's Adam: the MLP with the global step
 * count (`step`, advanced by the call on the device), the hash table by the non-matrix rule (rtxn_adam_step_sparse); every
 * gradient buffer is cleared as it is consumed, so they must be zero before the first call.
 * trace: the batch's rays (explicit or pinhole), grid and the per-ray outputs (num_hits, viewing_direction, sub_hits ...);
 *   its segment outputs are taken from `batch` (start_points, end_points, seg_view, num_stored, indices, segment_capacity).
 * batch: as rtxn_train_gradients; total_segments is written by the scan of this call. */
typedef struct rtxn_train_state {
  float* mlp_master;            /* float[rtxn_mlp_n_params]: fp32 master copy (main.cu:328-342) */
  void* mlp_params_fp16;        /* half[n]: the parameters the kernels read */
  float* mlp_m; float* mlp_v;   /* Adam moments */
  float* table_master; void* table_params_fp16; float* table_m; float* table_v;   /* hash grid only: the same for the table ... */
  unsigned* table_steps;        /* ... and its per-entry update counts (uint32[n], zero-initialised) */
  int* step;                    /* DEVICE int: optimisation steps taken so far; the call increments it */
  float* effective_lr;          /* DEVICE float scratch: the MLP's bias-corrected rate of this step */
  float lr, beta1, beta2, eps;  /* main.cu:36-46: 1e-3, 0.9, 0.999, 1e-8 */
  float table_lr, table_eps;    /* tcnn non_matrix_learning_rate_factor x lr; 1e-15 */
  float loss_scale_divisor;     /* 1, or the number of ranks whose gradients were summed into the buffers */
} rtxn_train_state;
typedef struct rtxn_train_step_args {
  rtxn_trace_params trace;
  void* scan_workspace;         /* rtxn_scan_workspace_bytes(batch.n_rays) */
  size_t scan_workspace_bytes;
  rtxn_train_batch batch;
  rtxn_train_state opt;
} rtxn_train_step_args;
int rtxn_train_step(const rtxn_train_step_args* args, rtxn_stream_t stream);
/* rtxn_train_step over a background (rtxn_train_gradients_ex).  RANDOM with bg->step == NULL hashes opt.step as it is BEFORE
 * this call increments it: a replayed graph of the call draws the backgrounds of step 0, 1, 2, ... */
int rtxn_train_step_ex(const rtxn_train_step_args* args, const rtxn_train_background* bg, rtxn_stream_t stream);

/* ---- segments that carry a loss gradient ---------------------------------------------------------------------------
 * In NeRF training most samples lie behind the first surface: their transmittance, and with it dL/d(radiance), is exactly
 * zero, and so is everything the backward pass would add for them.  rtxn_live_segments lists the 32-sample segments with a
 * non-zero radiance gradient (ascending segment indices + their count, in live_ws); the two _live entry points below are
 * rtxn_mlp_train_backward_recompute / rtxn_mlp_train_backward / rtxn_hashgrid_backward_segments visiting only those segments.  Same sums, fewer
 * terms: results equal to the unrestricted calls up to the order of fp32 / fp16 atomics.  d(encoding) is written for the
 * listed segments only (no reader of the other columns remains).  No counterpart in the reference (tiny-cuda-nn backpropagates
 * every sample). */
size_t rtxn_live_segments_workspace_bytes(long segment_capacity);
int rtxn_live_segments(const void* radiance_gradients_half4, long n_segments, long segment_capacity, void* live_ws,
                       rtxn_stream_t stream);
int rtxn_mlp_train_backward_recompute_live(const rtxn_mlp* m, const void* encT, const void* output_half,
                                           const void* dout_half4, long n_samples, const void* live_ws, float* dparams,
                                           void* dencT, rtxn_stream_t stream);
/* rtxn_mlp_train_backward (the saved-activation path, any built width) over the live segments: the chain visits only
 * them and writes their dZ compactly, the weight-gradient kernels contract over 32 * count samples. */
int rtxn_mlp_train_backward_live(const rtxn_mlp* m, const void* encT, const void* output_half, const void* dout_half4,
                                 long n_samples, void* workspace, const void* live_ws, float* dparams, void* dencT,
                                 rtxn_stream_t stream);
/* The saving half of network->forward over the live segments only: a step that has run rtxn_mlp_train_forward_outputs over
 * the whole batch (outputs, no activations), the compositor and rtxn_live_segments then saves the activations of just the
 * segments the backward will visit -- into the same workspace, at the same places rtxn_mlp_train_forward would have put them,
 * so rtxn_mlp_train_backward_live reads them unchanged.  (In NeRF training 70-90 % of a batch lies behind the first surface
 * and carries no gradient: the full saving forward is the largest kernel of the 8x128 step, and most of what it writes is
 * never read.) */
int rtxn_mlp_train_forward_live(const rtxn_mlp* m, const void* encT, long n_samples, void* workspace, const void* live_ws,
                                rtxn_stream_t stream);
int rtxn_hashgrid_backward_segments_live(const rtxn_hashgrid* g, const float* start_points, const float* end_points,
                                         long n_segments, int sample_type, const void* dencT, const void* live_ws,
                                         float* dtable, void* dtable_hashed_half, rtxn_stream_t stream);

/* ---- sample jitter (training only) ----------------------------------------------------------------------------------
 * RTXN_SAMPLING_JITTER_WORLD: stratified per-step jitter of the 32 samples of a segment (not in the reference, whose two random
 * modes replay one minstd_rand stream for every ray and step; NeRF's perturb / instant-ngp's per-step offsets).  Sample i of
 * packed segment g of the batch, s = 32 g + i:
 *   step = (uint32)*jitter.step (NULL: 0)
 *   h0   = fmix32((seed ^ 0x5BD1E995u) + 0x9E3779B9u * step)      (uint32 wrap-around; fmix32: see RTXN_BG_RANDOM)
 *   u    = (float)(fmix32(h0 ^ (uint32)s) >> 8) * 2^-24           (24 hash bits, exact, in [0, 1))
 *   t    = ((float)i + u) * (1/32)                                in [i/32, (i + 1)/32): inside its stratum and its cell
 *   pos  = fmaf(t, end - start, start),  (theta, phi) = the segment's
 *   t_vals[s] = |end - start| / 32 * t_scale                      exactly MIDPOINT_WORLD's
 * The offset is a pure function of (seed, step, s) and is never stored: the encoders, the lean forward and weight gradient and
 * the hash scatter (also over a live list) each form the same position from the same s, so the backward differentiates the
 * samples the forward shaded.  `step` is read on the device: a captured graph draws new offsets on every replay once the
 * counter moves, the same step number gives the same offsets on every path, and a resumed run continues the sequence.  The
 * step LENGTH stays the stratum's, so the compositor and its backward are untouched and remain exact.
 * Every entry point that reads packed segments for training has a `_jitter` form with the struct as its last argument before
 * the stream; the plain name is that form called with NULL.  Rules (RTXN_ERR_INVALID with a message, before any device is
 * touched): RTXN_SAMPLING_JITTER_WORLD needs the struct; the struct needs RTXN_SAMPLING_JITTER_WORLD; not with RTXN_VR_COMPAT
 * (rtxn_train_gradients_jitter / rtxn_train_step_jitter), whose t_vals are not step lengths.  Rendering and the occupancy
 * refresh stay deterministic: rtxn_render_*, rtxn_hashmlp_forward_segments, rtxn_volrender_fwd_aux and rtxn_sample refuse
 * type 4. */
typedef struct rtxn_sample_jitter {
  unsigned seed;
  const int* step;                  /* DEVICE int hashed with the seed; NULL = 0 (rtxn_train_step_jitter: NULL = opt.step before
                                       its increment) */
} rtxn_sample_jitter;
/* rtxn_sample with room for the jitter: the same positions and t_vals as float[S][5] / float[S] (s = the sample's index in the
 * packed batch).  sample_type 0..3 with jitter == NULL: rtxn_sample. */
int rtxn_sample_ex(const float* start_points, const float* end_points, const float* view_dirs,
                   float* t_vals, float* sampled_points, int batch_size, int grid_res,
                   const int* num_hits, const int* indices, int sample_type, const rtxn_sample_jitter* jitter,
                   rtxn_stream_t stream);
int rtxn_encode_frequency_segments_jitter(const rtxn_mlp* m, const float* start_points, const float* end_points,
                                          const float* seg_view, long n_segments, int sample_type, float t_scale,
                                          void* encT, float* t_vals, const rtxn_sample_jitter* jitter, rtxn_stream_t stream);
int rtxn_hashgrid_encode_segments_jitter(const rtxn_hashgrid* g, int n_dir_freqs, const void* table_fp16,
                                         const float* start_points, const float* end_points, const float* seg_view,
                                         long n_segments, int sample_type, float t_scale, void* encT, float* t_vals,
                                         const rtxn_sample_jitter* jitter, rtxn_stream_t stream);
int rtxn_mlp_train_forward_lean_segments_jitter(const rtxn_mlp* m, const float* start_points, const float* end_points,
                                                const float* seg_view, long n_segments, int sample_type, float t_scale,
                                                float* t_vals, void* workspace_lean, void* output_half, float* radiance,
                                                const rtxn_sample_jitter* jitter, rtxn_stream_t stream);
int rtxn_mlp_train_backward_lean_segments_jitter(const rtxn_mlp* m, const float* start_points, const float* end_points,
                                                 const float* seg_view, long n_segments, int sample_type, const void* output_half,
                                                 const void* dout_half4, void* workspace_lean, const void* live_ws, float* dparams,
                                                 const rtxn_sample_jitter* jitter, rtxn_stream_t stream);
int rtxn_hashgrid_backward_segments_jitter(const rtxn_hashgrid* g, const float* start_points, const float* end_points,
                                           long n_segments, int sample_type, const void* dencT, float* dtable,
                                           void* dtable_hashed_half, const rtxn_sample_jitter* jitter, rtxn_stream_t stream);
int rtxn_hashgrid_backward_segments_live_jitter(const rtxn_hashgrid* g, const float* start_points, const float* end_points,
                                                long n_segments, int sample_type, const void* dencT, const void* live_ws,
                                                float* dtable, void* dtable_hashed_half, const rtxn_sample_jitter* jitter,
                                                rtxn_stream_t stream);
/* rtxn_train_gradients_ex / rtxn_train_step_ex with the jitter beside the background; either may be NULL.  The step form: a
 * NULL jitter->step is opt.step as it is BEFORE the call increments it, by the background's rule. */
int rtxn_train_gradients_jitter(const rtxn_train_batch* batch, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                rtxn_stream_t stream);
int rtxn_train_step_jitter(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                           rtxn_stream_t stream);

/* ---- training losses beyond L2 (not in the reference, whose loss is tcnn "L2", main.cu:36-38) ---------------------------
 * Per ray r:
 *   pixel  p_c = sum_k w_k c_kc + (1 - A) b_c, with A = sum_k w_k;
 *   target t_c is the ray's target, RGBA composited over the ray's background (as rtxn_volrender_l2_train_ex does);
 *   e_c = p_c - t_c;
 *   N = 3 n_rays.
 *
 *   kind                                      | per-channel term l(e)                              | dl/dp
 *   RTXN_LOSS_L2 = 0                          | e^2                                                | 2e
 *   RTXN_LOSS_L1 = 1                          | abs(e)                                             | sign(e), 0 at e == 0
 *   RTXN_LOSS_HUBER = 2 (param = delta > 0)   | e^2 / 2 if abs(e) <= delta,                        | clamp(e, -delta, delta)
 *                                             | else delta (abs(e) - delta / 2)                    |
 *   RTXN_LOSS_RELATIVE_L2 = 3 (param = eps>0) | e^2 / (p^2 + eps)                                  | 2e / (p^2 + eps)
 *
 * For relative L2 the denominator is a constant to the gradient, as in tiny-cuda-nn.  The division is IEEE.
 * Alpha term, weight lambda = opacity_weight >= 0: lambda (A - alpha_r)^2 per ray, where alpha_r is the target's fourth
 * channel.  So lambda > 0 needs 4-channel targets and the RTXN_VR_NERF compositor.
 * The loss scalar written to loss_sum, unscaled:
 *   (1/N) sum l(e) + (lambda / n_rays) sum (A - alpha)^2
 * The gradients handed on, each rounded to fp16 exactly as the L2 path rounds its own and used in that rounded form:
 *   g_c = half(loss_scale l'(e_c) / N)
 *   g_A = half(loss_scale lambda 2 (A - alpha) / n_rays)
 * Sweep 2 is the background kernels' sweep with one more constant:
 *   dL/dw_k = g.c_k - g.b + g_A, so gc = (g.c_k) - gbg + g_A;
 *   S = g.(sum w c) - gbg A + g_A A;
 *   with no background, b = 0 and gbg = 0.
 * Rules (RTXN_ERR_INVALID with a message naming the field, before any device is touched): a known kind; HUBER and
 * RELATIVE_L2 need a finite param > 0; opacity_weight >= 0; opacity_weight > 0 needs 4-channel targets (a CONSTANT or RANDOM
 * background) and not RTXN_VR_COMPAT.  In deterministic mode (rtxn_set_deterministic_workspace) the scalar is summed in a
 * fixed order behind the compositor from pixels, targets and, with opacity_weight > 0, the opacities: `opacity` must then be
 * given.  loss == NULL, or kind L2 with opacity_weight == 0 and opacity == NULL: exactly the call without the struct -- the
 * same kernels, the same bits. */
enum rtxn_loss_kind { RTXN_LOSS_L2 = 0, RTXN_LOSS_L1 = 1, RTXN_LOSS_HUBER = 2, RTXN_LOSS_RELATIVE_L2 = 3 };
typedef struct rtxn_train_loss {
  int kind;               /* rtxn_loss_kind */
  float param;            /* HUBER: delta; RELATIVE_L2: epsilon; otherwise ignored */
  float opacity_weight;   /* lambda */
  float* opacity;         /* optional DEVICE float[n_rays]: A of every ray, written by the compositor; NULL: not written */
} rtxn_train_loss;
/* rtxn_volrender_l2_train_ex with the loss chosen by `loss` (bg may be NULL: black, 3-channel targets) */
int rtxn_volrender_loss_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                              int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                              void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                              const rtxn_train_background* bg, const rtxn_train_loss* loss, rtxn_stream_t stream);
/* rtxn_l2_loss for the four kinds, elementwise with N = n: values[i] = l(e_i) / n, grads[i] = half(loss_scale l'(e_i) / n),
 * *loss_sum = sum of values (a float atomic per block).  What the RTXN_VR_COMPAT three-launch route of rtxn_train_gradients_loss
 * uses.  opacity_weight must be 0 and opacity NULL: there is no compositor here. */
int rtxn_loss(const float* pred, const float* target, long n, const rtxn_train_loss* loss, float loss_scale, float* values,
              void* grads_half, float* loss_sum, rtxn_stream_t stream);
/* rtxn_train_gradients_jitter / rtxn_train_step_jitter with the loss beside the background and the jitter; each may be NULL.
 * The step form: a NULL bg->step or jitter->step is opt.step as it is BEFORE the call increments it. */
int rtxn_train_gradients_loss(const rtxn_train_batch* batch, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                              const rtxn_train_loss* loss, rtxn_stream_t stream);
int rtxn_train_step_loss(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                         const rtxn_train_loss* loss, rtxn_stream_t stream);

/* ---- distortion regulariser (mip-NeRF 360; not in the reference) -----------------------------------------------------------
 * Per ray r, over its n = num_samples_per_hit * num_stored samples in storage order (a ray's segments are stored in ascending,
 * disjoint t):
 *   w_i     the RTXN_VR_NERF compositor's weights, exactly those the pixel uses;
 *   delta_i = (t_end_j - t_start_j) * (1 / K), the width of sub-interval k of segment j: the step length the compositor reads
 *           (ray_hit / t_vals) wherever that is a distance -- rtxn_train_batch.t_scale is a factor on sigma that the step lengths
 *           of a batch carry, and no part of delta_i;
 *   m_i     = fmaf((k + 0.5) * (1 / K), t_end_j - t_start_j, t_start_j), the midpoint of sub-interval k of segment j (K samples
 *           per segment) -- the depth expression of rtxn_volrender_fwd_aux with u0 = 0.5.  With RTXN_SAMPLING_JITTER_WORLD m_i
 *           stays the stratum's midpoint and delta_i its width: w_i is taken as the weight of the interval, not of the
 *           jittered point, so the compositor needs no jitter state.
 *   L_r   = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i
 *         = 2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 delta_i,    W_<i = sum_{j<i} w_j,  M_<i = sum_{j<i} w_j m_j
 *   q_i   = dL_r/dw_i = 2 [m_i (W_<i - W_>i) - (M_<i - M_>i)] + (2/3) w_i delta_i
 *   loss += (lambda_d / n_rays) sum_r L_r                                  (lambda_d = distortion_weight)
 * Distances are world units along the normalised ray; the cube [-1, 1]^3 has diagonal 2 sqrt(3), so a lambda quoted for
 * distances normalised to [0, 1] is divided by that.
 * The term enters sweep 2 (see the losses above) as one more addend of gc, with k = loss_scale lambda_d / n_rays in fp32 -- no
 * fp16 hand-off for this term:
 *   dL/dw_i = g.c_i - g.b + g_A + k q_i;     S gains 2 k L_r   (sum_i w_i q_i = 2 L_r: L_r is homogeneous of degree 2 in w).
 * The radiance gradients are fp16: with loss_scale 128, 4096 rays and lambda_d = 0.01 the term is ~1e-7 per sample, one or two
 * fp16 subnormal steps, and is largely rounded away on its own; it needs a larger loss_scale to act where the colour gradient
 * has vanished.
 * Rules (RTXN_ERR_INVALID with a message naming the field, before any device is touched): distortion_weight finite and >= 0;
 * a weight > 0, or either output pointer, needs t_start and t_end, the RTXN_VR_NERF compositor and sample_type
 * RTXN_SAMPLING_MIDPOINT_WORLD or RTXN_SAMPLING_JITTER_WORLD.  In deterministic mode the scalar is summed in a fixed order
 * behind the compositor; with distortion_weight > 0 that sum reads `distortion`, which must then be given (the rule `opacity`
 * follows).  reg == NULL, or weight 0 with both outputs NULL: exactly the corresponding _loss call -- the same kernels, the same
 * bits. */
typedef struct rtxn_train_regularizer {
  float distortion_weight;   /* lambda_d >= 0, finite */
  const float* t_start;      /* DEVICE float per packed segment slot, as rtxn_trace_grid writes them (RTXN_TRACE_DDA) */
  const float* t_end;
  float* distortion;         /* optional DEVICE float[n_rays]: L_r of every ray */
  float* depth;              /* optional DEVICE float[n_rays]: sum w_i m_i (rtxn_volrender_fwd_aux's depth for MIDPOINT_WORLD) */
} rtxn_train_regularizer;
/* rtxn_volrender_loss_train with the regulariser (bg and loss may be NULL) */
int rtxn_volrender_reg_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                             int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                             void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                             const rtxn_train_background* bg, const rtxn_train_loss* loss, const rtxn_train_regularizer* reg,
                             rtxn_stream_t stream);
/* rtxn_train_gradients_loss / rtxn_train_step_loss with the regulariser beside the other three; each may be NULL.  The step
 * form traces in RTXN_TRACE_DDA (RTXN_TRACE_COMPAT is refused when the regulariser is active) and its write pass stores the
 * segments' t_start / t_end into the struct's buffers, which must hold batch.segment_capacity floats each. */
int rtxn_train_gradients_reg(const rtxn_train_batch* batch, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                             const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, rtxn_stream_t stream);
int rtxn_train_step_reg(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                        const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, rtxn_stream_t stream);

/* ---- optimizer options: learning-rate schedule, decoupled weight decay, non-finite guard -------------------------------
 * Not in the reference, whose configuration only says what it wanted (main.cu:39, "adam optimizer decays from 5e-4 to 5e-5").
 * Everything is evaluated ON THE DEVICE from the step counter, so a captured step needs nothing refreshed from the host.
 * With t the 1-based number of the update (the device step counter AFTER this step's increment; rtxn_adam_step's `step`):
 *   warm(t) = warmup_steps > 0 ? min(1, t / warmup_steps) : 1
 *   x(t)    = max(0, t - decay_start) / decay_steps                  (staircase: floor(x))
 *   RTXN_LR_CONSTANT:     dec = 1
 *   RTXN_LR_EXPONENTIAL:  dec = ratio^x                              (unbounded)
 *   RTXN_LR_COSINE:       dec = ratio + (1 - ratio) (1 + cos(pi min(x, 1))) / 2     (ratio: the final factor)
 *   factor(t) = (float)(warm dec)     -- all of it in double ((double)ratio), rounded to float once
 *   lr_t = lr factor(t),  table_lr_t = table_lr factor(t)            (float products)
 * The MLP's bias-corrected rate is rtxn_adam_effective_lr's expression with lr_t for lr; the table's sparse Adam uses table_lr_t
 * for its lr.  RTXN_LR_CONSTANT without warm-up is exactly 1.0f.
 * weight_decay (AdamW, decoupled): after the Adam update of an element, w -= lr_t weight_decay w, with lr_t the scheduled rate
 * WITHOUT bias correction.  The step entry point applies it to the MLP only (tiny-cuda-nn regularises matrix parameters only).
 * skip_nonfinite: rtxn_check_gradients ORs guard[0] if any element of the gradient buffers the optimizer is about to consume is
 * Inf or NaN; rtxn_optimizer_rate moves that into the skip word guard[2], clears guard[0] and counts guard[1] up; the _opt Adam
 * kernels read the skip word before any store to the state: master weights, fp16 parameters, both moments and the table's
 * per-entry counts keep their bits, the gradient is still cleared (RTXN_ADAM_ZERO_GRADS).  The step counter advances all the
 * same -- it keys the sample jitter, the random background and this schedule -- so Adam's global bias-correction step counts
 * ATTEMPTED steps.  The loss scale of these entry points is a by-value argument and stays what it is; rtxn_loss_scaler, below,
 * keeps it in device memory and lowers it when a step is skipped.
 * Rules (RTXN_ERR_INVALID with a message, before any device is touched): kind is one of the three; ratio in (0, 1];
 * decay_steps >= 1 unless the kind is CONSTANT; warmup_steps >= 0 and decay_start >= 0; staircase only with EXPONENTIAL;
 * weight_decay finite and >= 0; when anything is switched on, lr_factor, and with skip_nonfinite guard, must not be NULL.
 * "Switched on": a schedule other than CONSTANT without warm-up, weight_decay > 0 or skip_nonfinite != 0.  With NULL options,
 * or nothing switched on, every _opt entry point makes exactly the call that existed before it. */
enum rtxn_lr_schedule_kind { RTXN_LR_CONSTANT = 0, RTXN_LR_EXPONENTIAL = 1, RTXN_LR_COSINE = 2 };
typedef struct rtxn_lr_schedule {
  int kind;                         /* rtxn_lr_schedule_kind */
  int warmup_steps;                 /* linear warm-up over the first warmup_steps updates; 0: none */
  int decay_start;                  /* the decay's x is 0 up to this update */
  int decay_steps;                  /* updates per unit of x */
  float ratio;                      /* EXPONENTIAL: factor per decay_steps; COSINE: the final factor */
  int staircase;                    /* EXPONENTIAL only: x = floor(x) */
} rtxn_lr_schedule;
typedef struct rtxn_optimizer_options {
  rtxn_lr_schedule schedule;
  float weight_decay;
  int skip_nonfinite;
  float* lr_factor;                 /* DEVICE float scratch: factor(t) of this step, written by rtxn_optimizer_rate */
  unsigned* guard;                  /* DEVICE unsigned[4], zero-initialised: [0] the non-finite flag, [1] skipped steps so far,
                                       [2] this step's skip word, [3] unused; may be NULL without skip_nonfinite */
} rtxn_optimizer_options;
/* factor(t) on the host: the definition above (step < 1, or a schedule that breaks the rules: -1 and a message;
 * a factor is never negative). */
float rtxn_lr_schedule_factor(const rtxn_lr_schedule* schedule, int step);
/* The rules above without the two pointers (what a caller checks before it allocates anything); NULL is valid. */
int rtxn_optimizer_options_check(const rtxn_optimizer_options* opt);
/* The one-thread rate kernel every stepping path shares: t = *step (+ 1, written back, if advance != 0);
 * *opt->lr_factor = factor(t); *effective_lr = lr_t sqrt(1 - beta2^t) / (1 - beta1^t); *table_effective_lr (may be NULL): the
 * same with table_lr_t, for a table stepped by the dense rule; with skip_nonfinite the guard words move as described above.
 * The powers, the cosine and warm dec are formed in double and rounded once, so the device's value is the host's to an ulp. */
int rtxn_optimizer_rate(const rtxn_optimizer_options* opt, int* step, int advance, float lr, float table_lr, float beta1, float beta2,
                        float* effective_lr, float* table_effective_lr, rtxn_stream_t stream);
/* ORs *flag (device unsigned, opt->guard) with 1 if any element of up to RTXN_MAX_GRAD_BUFFERS gradient buffers is Inf or NaN:
 * one launch, 16 bytes per lane, the exponent bits tested on the raw words, at most one atomic per wave.  An OR is order-free:
 * deterministic mode stays deterministic.  Buffers with count 0 are skipped. */
enum { RTXN_MAX_GRAD_BUFFERS = 4 };
typedef struct rtxn_grad_buffer {
  const void* data;                 /* DEVICE float[count] or half[count] */
  long count;
  int is_fp16;
} rtxn_grad_buffer;
int rtxn_check_gradients(const rtxn_grad_buffer* buffers, int n_buffers, unsigned* flag, rtxn_stream_t stream);
/* rtxn_adam_step_captured / rtxn_adam_step_sparse under the options: the rate is *effective_lr (dense; rtxn_optimizer_rate
 * wrote it) or lr * *opt->lr_factor (sparse), the decay term uses lr * *opt->lr_factor, and with skip_nonfinite the skip word
 * is honoured.  grad_flags: as rtxn_adam_step_captured, and RTXN_ADAM_NO_WEIGHT_DECAY: opt->weight_decay is not applied by
 * this call (the hash table).  The sparse form decays the entries it updates.  opt == NULL or nothing switched on: the call
 * without _opt (the dense one ignores `lr` then). */
enum { RTXN_ADAM_NO_WEIGHT_DECAY = 4 };
int rtxn_adam_step_opt(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                       const float* effective_lr, float lr, float beta1, float beta2, float eps, float loss_scale,
                       const rtxn_optimizer_options* opt, rtxn_stream_t stream);
int rtxn_adam_step_sparse_opt(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                              unsigned* param_steps, float lr, float beta1, float beta2, float eps, float loss_scale,
                              const rtxn_optimizer_options* opt, rtxn_stream_t stream);
/* rtxn_train_step_reg under the options (each of the four other structs may be NULL): behind the gradients, rtxn_check_gradients
 * over dparams, dtable[:hashed_lo] and dtable_hashed_half (or the whole fp32 dtable) with skip_nonfinite, then rtxn_optimizer_rate
 * advancing args->opt.step, then the _opt Adam calls -- weight decay on the MLP only. */
int rtxn_train_step_opt(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                        const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                        rtxn_stream_t stream);

/* ---- dynamic loss scale and gradient-norm clipping (not in the reference) ------------------------------------
 * The loss scale lives in device memory and the factor the optimizer multiplies raw gradients by lives beside it, so a captured
 * or one-call step adapts the scale without anything refreshed from the host.  The scale enters a step in one place, the
 * compositor's per-ray step (the fp16 loss gradients, g_A and the regulariser's k), and leaves it in one place, the factor of
 * the Adam kernels; everything between just carries it.
 * Device state (rtxn_loss_scaler_state, 8 words): scale -- what the NEXT compositor launch reads; multiplier -- what this
 * step's Adam kernels multiply raw gradients by; good -- clean steps since the last change; the counters backoffs, growths,
 * clipped; grad_norm -- the last clean step's unscaled total norm.  The skipped-step count stays in opt->guard[1].
 * Per step, once the gradients are complete, with s the scale they were made with, D = loss_scale_divisor (ranks summed) and
 * sumsq the sum of squares, in double, of every gradient element the optimizer is about to consume (MLP and table together):
 *   non-finite flag set:  the skip word is set (as rtxn_optimizer_rate does); scale = max(min_scale, s backoff); good = 0;
 *                         backoffs += 1.  At min_scale the step is still skipped: a NaN from the data is not the scale's fault.
 *   flag clear:           norm = (float)(sqrt(sumsq) / ((double)s (double)D))
 *                         coef = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6f)) : 1     (clip_grad_norm_'s rule)
 *                         multiplier = coef (1.0f / (s D))   -- float; coef == 1 gives exactly 1.0f / (s D)
 *                         grad_norm = norm; clipped += (coef < 1); good += 1;
 *                         good >= growth_interval: scale = min(max_scale, s growth), good = 0, growths += 1 if the scale moved.
 * The step counter advances either way.  Scales and factors are powers of two, so multiplying by them is exact in fp32: a run
 * whose scale never moves and that never clips is the fixed-scale run under skip_nonfinite, bit for bit.
 * Rules (RTXN_ERR_INVALID with a message, before any device is touched): init_scale, growth, backoff, min_scale and max_scale
 * are exact powers of two; min_scale <= init_scale <= max_scale; growth >= 1; 0 < backoff < 1; growth_interval >= 1;
 * max_grad_norm finite and >= 0 (0: no clipping).  The entry points that take the struct also need `state` and `partials`, and
 * options with skip_nonfinite, lr_factor and guard: dynamic scaling implies the non-finite guard.  RTXN_VR_NERF only. */
typedef struct rtxn_loss_scaler_state {
  float scale;
  float multiplier;
  int good;
  unsigned backoffs, growths, clipped;
  float grad_norm;
  int reserved;
} rtxn_loss_scaler_state;
enum { RTXN_GRAD_STATS_MAX_BLOCKS = 2048 };
typedef struct rtxn_loss_scaler {
  float init_scale;
  float growth;                     /* default 2 */
  float backoff;                    /* default 0.5 */
  int growth_interval;              /* clean steps between two growths; default 2000 */
  float min_scale;                  /* default 1 */
  float max_scale;                  /* default 65536 */
  float max_grad_norm;              /* 0: no clipping */
  rtxn_loss_scaler_state* state;    /* DEVICE, initialised from rtxn_loss_scaler_init_state */
  double* partials;                 /* DEVICE workspace of rtxn_loss_scaler_workspace_bytes() bytes: per-block sums of squares,
                                       [RTXN_MAX_GRAD_BUFFERS][RTXN_GRAD_STATS_MAX_BLOCKS] */
} rtxn_loss_scaler;
/* The rules above without the two pointers (what a caller checks before it allocates anything). */
int rtxn_loss_scaler_check(const rtxn_loss_scaler* scaler);
size_t rtxn_loss_scaler_workspace_bytes(void);
/* HOST: the state a run starts from (scale = init_scale, multiplier = 1 / init_scale, everything else 0), to be copied to
 * scaler->state. */
int rtxn_loss_scaler_init_state(const rtxn_loss_scaler* scaler, rtxn_loss_scaler_state* state_out);
/* HOST twin of the device state machine, on the restatement both share: *state_out = the state after a step whose gradients
 * were made with state_in->scale, with the non-finite flag `flag`, the sum of squares `sumsq` and the divisor D. */
int rtxn_loss_scaler_advance(const rtxn_loss_scaler* scaler, const rtxn_loss_scaler_state* state_in, int flag, double sumsq,
                             float divisor, rtxn_loss_scaler_state* state_out);
/* rtxn_check_gradients' pass plus the norm: ORs *flag as it does, and stores one double sum of squares per block at
 * scaler->partials[buffer][block].  A buffer's blocks, and the elements each lane visits, are a pure function of that buffer's
 * count, element type and alignment; a lane sums in double in visiting order, a wave and then a block reduce in a fixed order
 * and no atomic touches the sums: the same bits run to run, in or out of deterministic mode, alone or beside other buffers. */
int rtxn_gradient_statistics(const rtxn_grad_buffer* buffers, int n_buffers, unsigned* flag, const rtxn_loss_scaler* scaler,
                             rtxn_stream_t stream);
/* rtxn_optimizer_rate's sibling, one block: reduces the partials rtxn_gradient_statistics left for these same buffers (only
 * their counts and types are read here) in a fixed tree, does everything rtxn_optimizer_rate does and then moves
 * scaler->state as stated above with D = divisor.  Every stepping path launches this one kernel. */
int rtxn_loss_scaler_step(const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_grad_buffer* buffers,
                          int n_buffers, int* step, int advance, float lr, float table_lr, float beta1, float beta2,
                          float* effective_lr, float* table_effective_lr, float divisor, rtxn_stream_t stream);
/* rtxn_adam_step_opt / rtxn_adam_step_sparse_opt with the factor on the raw gradient read from scaler->state->multiplier
 * instead of formed from a loss_scale argument; everything else is those calls. */
int rtxn_adam_step_scaled(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                          const float* effective_lr, float lr, float beta1, float beta2, float eps,
                          const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, rtxn_stream_t stream);
int rtxn_adam_step_sparse_scaled(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                                 unsigned* param_steps, float lr, float beta1, float beta2, float eps,
                                 const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, rtxn_stream_t stream);
/* rtxn_volrender_reg_train reading the loss scale from scaler->state->scale (one scalar load per wave); `loss_scale` is then
 * ignored.  Always the loss compositor's kernels, plain L2 included (bg, loss and reg may each be NULL).  scaler == NULL:
 * exactly rtxn_volrender_reg_train. */
int rtxn_volrender_scaled_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                                int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                                void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                                const rtxn_train_background* bg, const rtxn_train_loss* loss, const rtxn_train_regularizer* reg,
                                const rtxn_loss_scaler* scaler, rtxn_stream_t stream);
/* rtxn_train_gradients_reg with the scaler: batch->loss_scale is ignored, the compositor reads the device word.
 * batch->vr_mode must be RTXN_VR_NERF.  scaler == NULL: exactly rtxn_train_gradients_reg. */
int rtxn_train_gradients_scaled(const rtxn_train_batch* batch, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                                const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_loss_scaler* scaler,
                                rtxn_stream_t stream);
/* rtxn_train_step_opt with the scaler: gradients, rtxn_gradient_statistics over the buffers rtxn_train_step_opt checks,
 * rtxn_loss_scaler_step with D = args->opt.loss_scale_divisor, scaled Adam on the MLP, the training-weight re-pack, scaled
 * Adam on the table -- all on `stream`, so the next step's compositor is ordered behind this step's scaler kernel.
 * scaler == NULL: exactly rtxn_train_step_opt. */
int rtxn_train_step_scaled(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                           const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                           const rtxn_loss_scaler* scaler, rtxn_stream_t stream);

/* ---- exponential moving average of the weights (tiny-cuda-nn's EMA optimizer) ------------------------------
 * d: the decay, 0 < d < 1.  u: the number of APPLIED updates, a device word (state->updates); a step the non-finite guard skips
 * does not advance it.  Per parameter an accumulator s, fp32, zero at the start.  After Adam's update number u has written w_u:
 *   s_u = d s_{u-1} + (1 - d) w_u                 -- float: two products and a sum, 1 - d formed once on the host
 *   read-out:  w_ema = s_u correction(u),   correction(u) = (float)(1 / (1 - d^u))   -- in double ((double)d), rounded once
 *              u = 0: w_ema = w, and correction(0) = 1
 * (the debiased form: the initial weights carry no weight of their own).  The rate kernel advances u behind its other work,
 * unless this step's skip word is set, and stores correction(u) beside it.
 * DENSE form (the MLP; a table stepped by the dense rule): the line above for every element, in the Adam kernel, behind the
 * weight-decay term.
 * LAZY form (a table under the sparse rule, whose kernel leaves an element with a zero gradient untouched): a stamp e per
 * parameter (uint32, zero at the start) holds the u at which s was last current.  Between two touches w is a constant, and over a
 * constant the recurrence has a closed form: catch_up(s, w, gap) = gap == 0 ? s : fma(d^gap, s - w, w), with
 * d^gap = exp2((float)gap * (float)log2((double)d)) -- gap == 0 returns s itself, bit for bit.  When the sparse kernel updates an
 * element at update u (g != 0), with w_old read before Adam:
 *   s = catch_up(s, w_old, u - 1 - e);   s = d s + (1 - d) w_new;   e = u
 * The read-out is catch_up(s, w, u - e) correction(u) and is PURE: it stores neither s nor e, so rendering in the middle of a
 * run does not change a bit of the training state.  An entry never touched reads out as its weight (to the roundings of the
 * fma, the exp2 and the product).  A skipped step stores nothing to s, e, updates or correction; gradients are still cleared.
 * Rules (RTXN_ERR_INVALID with a message, before any device is touched): decay finite and strictly inside (0, 1).  The entry
 * points that take the struct also need `state`, and options (opt != NULL) with lr_factor -- and guard with skip_nonfinite --
 * whether or not anything else is switched on: under the EMA a step always takes its rate from the rate kernel.  The EMA does
 * not switch the guard on. */
typedef struct rtxn_ema_state {
  unsigned updates;                 /* u */
  float correction;                 /* correction(u), written by the rate kernel */
  unsigned reserved[2];
} rtxn_ema_state;
typedef struct rtxn_weight_ema {
  float decay;
  rtxn_ema_state* state;            /* DEVICE, zero-initialised */
  float* mlp_ema;                   /* DEVICE float[n MLP parameters], zero-initialised: s, dense form */
  float* table_ema;                 /* DEVICE float[n table parameters], zero-initialised; NULL without a hash grid */
  unsigned* table_stamps;           /* DEVICE unsigned[n table parameters], zero-initialised: e, lazy form; NULL: dense form */
} rtxn_weight_ema;
/* The rules above without the pointers (what a caller checks before it allocates anything); NULL is valid. */
int rtxn_weight_ema_check(const rtxn_weight_ema* ema);
/* HOST twins of the device arithmetic, on the restatement both share.  rtxn_ema_catch_up: catch_up(s, w, gap) above (a decay
 * outside (0, 1): NaN and a message).  rtxn_ema_correction: correction(updates); updates = 0 gives 1.0f (-1 and a message for
 * a decay outside (0, 1)). */
float rtxn_ema_catch_up(float s, float w, unsigned gap, float decay);
float rtxn_ema_correction(float decay, unsigned updates);
/* rtxn_optimizer_rate / rtxn_loss_scaler_step -- the same kernels -- that behind their work advance ema->state: one update of
 * the average per call that advances the step counter (advance != 0) and is not skipped; with advance == 0 the state keeps its
 * bits.  ema == NULL: exactly those calls.  opt may have nothing switched on but must carry lr_factor. */
int rtxn_optimizer_rate_ema(const rtxn_optimizer_options* opt, const rtxn_weight_ema* ema, int* step, int advance, float lr, float table_lr,
                            float beta1, float beta2, float* effective_lr, float* table_effective_lr, rtxn_stream_t stream);
int rtxn_loss_scaler_step_ema(const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema,
                              const rtxn_grad_buffer* buffers, int n_buffers, int* step, int advance, float lr, float table_lr, float beta1,
                              float beta2, float* effective_lr, float* table_effective_lr, float divisor, rtxn_stream_t stream);
/* rtxn_adam_step_scaled / rtxn_adam_step_sparse_scaled that also keep the average of the n parameters they step: ema_acc is
 * their s (dense form), ema_stamps their e (the sparse call: lazy form, required).  scaler == NULL: the factor on the raw
 * gradient is 1 / loss_scale, as rtxn_adam_step_opt forms it (with a scaler loss_scale is ignored).  The sparse kernel loads s
 * and e only for the quads whose gradient is not zero.  ema == NULL: exactly the _scaled call, or with scaler == NULL the _opt
 * call. */
int rtxn_adam_step_ema(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                       const float* effective_lr, float lr, float beta1, float beta2, float eps, float loss_scale,
                       const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, float* ema_acc,
                       rtxn_stream_t stream);
int rtxn_adam_step_sparse_ema(long n, float* master, void* params_fp16, void* grads, int grad_flags, float* m, float* v,
                              unsigned* param_steps, float lr, float beta1, float beta2, float eps, float loss_scale,
                              const rtxn_optimizer_options* opt, const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema,
                              float* ema_acc, unsigned* ema_stamps, rtxn_stream_t stream);
/* The read-out of n parameters: out_f32 and / or out_f16 (DEVICE, either may be NULL, not both) = the debiased average;
 * stamps == NULL: the dense form.  Reads master, ema_acc, stamps and state; stores only the outputs. */
int rtxn_ema_weights(long n, const float* master, const float* ema_acc, const unsigned* stamps, const rtxn_ema_state* state, float decay,
                     float* out_f32, void* out_f16, rtxn_stream_t stream);
/* rtxn_train_step_scaled's sequence (scaler == NULL: rtxn_train_step_opt's) with the _ema rate kernel call and the _ema Adam
 * calls in their slots: ema->mlp_ema for the MLP, ema->table_ema and ema->table_stamps (both required with a hash grid: this
 * call steps the table by the sparse rule) for the table.  ema == NULL: exactly rtxn_train_step_scaled. */
int rtxn_train_step_ema(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                        const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                        const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, rtxn_stream_t stream);

/* fp32 <-> fp16 copies of a gradient block on the device (no counterpart in the reference, which is single-GPU): the
 * data-parallel exchange sends the hashed levels' gradient in fp16 -- tiny-cuda-nn holds that gradient in fp16 throughout. */
int rtxn_convert_f32_to_f16(const float* src, void* dst_half, long n, rtxn_stream_t stream);
int rtxn_convert_f16_to_f32(const void* src_half, float* dst, long n, rtxn_stream_t stream);

/* ---- sparse view of a half2 gradient (data-parallel exchange; no counterpart in the single-GPU reference) ----
 * `values` is half2[n_entries] (the hashed levels' gradient: one entry = both features of a grid corner), cut into blocks of
 * block_entries entries (one hash-grid level each).  A rank's batch touches 0.2 % .. 25 % of a 2^19-entry level, so a level
 * is exchanged as (index, half2) pairs where that is smaller than the level: count, let the ranks agree per block, pack the
 * chosen blocks, gather the lists, add every rank's list (the rank's own included, in rank order) into the cleared blocks.
 *   rtxn_half2_count_nonzero: workspace (rtxn_half2_workspace_bytes) begins with int counts[ceil(n_entries / block_entries)]
 *     = entries of each block with a non-zero half; behind them the per-wave counts the pack pass places its entries with.
 *   rtxn_half2_pack_nonzero:  pairs (device uint32[capacity][2]: entry index, half2 bits) of the non-zero entries of the blocks
 *     whose bit is set in block_mask (at most 64 blocks), in ascending index; `workspace` as rtxn_half2_count_nonzero left it
 *     for these same values (no global append counter: one address takes ~10 ns per atomic).  *count (device int) = entries
 *     needed, which may exceed capacity (the list is then cut off: size it from the counts).  clear != 0: the selected blocks
 *     are left zero.
 *   rtxn_half2_add_pairs:     values[index] += value for `count` pairs (indices unique within a list; out-of-range ones are
 *     ignored); fp16 adds. */
size_t rtxn_half2_workspace_bytes(long n_entries, long block_entries);
int rtxn_half2_count_nonzero(const void* values, long n_entries, long block_entries, void* workspace, rtxn_stream_t stream);
int rtxn_half2_pack_nonzero(void* values, long n_entries, long block_entries, const void* workspace, unsigned long long block_mask,
                            long capacity, void* pairs, int* count, int clear, rtxn_stream_t stream);
int rtxn_half2_add_pairs(void* values, long n_entries, const void* pairs, long count, rtxn_stream_t stream);

/* ---- dataset loader (host only) ------------------------------------------------------- */
/* Replaces load_images_json (loader/data_loader.cpp:34-94; jsoncpp + stb_image's stbi_loadf).
 * Reads <basename>/transforms_<split>.json and its PNG frames.  images: float[n][H][W][3],
 * poses: float[n][16] row-major 4x4 (both malloc'ed, host).  flags = 0 reproduces the reference
 * (alpha dropped without compositing, gamma-2.2 linearisation, focal = .5*800/tan(.5*camera_angle_x),
 * SURVEY Q11/Q12); bit 0: composite alpha over white; bit 1: keep v/255 (no gamma); bit 2 (RTXN_LOAD_RGBA): images are
 * float[n][H][W][4] and image_channels = 4 -- RGB exactly as without bit 2, alpha = a/255 (no gamma, as stb treats alpha),
 * 1 for files without alpha; together with bit 0 it is an error. */
enum { RTXN_LOAD_RGBA = 4 };
typedef struct rtxn_image_dataset {
  int n_images;
  unsigned image_width, image_height, image_channels;
  float focal;
  float camera_angle_x;
  float* images;
  float* poses;
} rtxn_image_dataset;
int rtxn_load_images_json(const char* basename, const char* split, int flags, rtxn_image_dataset* out);
void rtxn_free_image_dataset(rtxn_image_dataset* d);
/* Fills the stub at loader/data_loader.cpp:140-142 (SceneType::LLFF: the reference sets the directory name and returns an
 * empty vector).  Reads <basedir>/poses_bounds.npy (float64[N][17]: row-major 3x5 [R | t | (H, W, focal)] in LLFF's
 * (down, right, back) axes + near/far bounds) and the PNG frames of <basedir>/images_<factor>/ (images/ if factor <= 1)
 * in name order.  poses: float[N][16] row-major camera-to-world, axes (right, up, back) like the synthetic loader's;
 * focal is in pixels of the loaded resolution; *bounds (may be NULL): malloc'ed float[N][2] near/far, release with
 * rtxn_free_llff_bounds.  flags as rtxn_load_images_json. */
int rtxn_load_llff(const char* basedir, int factor, int flags, rtxn_image_dataset* out, float** bounds);
void rtxn_free_llff_bounds(float* bounds);
/* stb_image_write's role (included, never called, main.cu:19-21): 8-bit RGB PNG of a rendered frame. */
int rtxn_write_png_rgb8(const char* path, const unsigned char* rgb, int width, int height);
/* A depth map: a gray PNG as uint16 [height][width] (malloc'd; rtxn_free_png_gray16), in the file's own unit.  16-bit samples
 * keep both bytes, 8-bit samples are widened as v (not v * 257); interlaced or not; a tRNS colour key is ignored.  Any other
 * colour type, and gray below 8 bits, is refused with a message (RTXN_ERR_IO, as every unreadable file). */
int rtxn_load_png_gray16(const char* path, int* width, int* height, uint16_t** values);
void rtxn_free_png_gray16(uint16_t* values);

/* ---- training batches drawn on the device --------------------------------------------------------------------------
 * Replaces the reference's host batch build (a random shuffle + gather, main.cu:612-629) and the per-ray dataset it
 * gathers from: the training frames stay resident as they were loaded (float, or one byte per channel) beside their poses,
 * and ONE kernel draws a batch -- picks (image, pixel) per ray, generates the pixel's pinhole ray and copies its colour --
 * on `stream`, without an allocation or a synchronisation, so the call is hipGraph-capturable in front of a traversal.
 * Batch number `step` (uint32 wrap-around throughout; fmix32: see RTXN_BG_RANDOM) draws, for ray r of n_rays:
 *   h0    = fmix32((seed ^ 0x2C1B3C6Du) + 0x9E3779B9u * (uint32)step)                 step = *step, NULL: 0
 *   image = (uint64(fmix32(h0 ^ (2r)))     * n_images)       >> 32
 *   pixel = (uint64(fmix32(h0 ^ (2r + 1))) * (width*height)) >> 32                    px = pixel % width, py = pixel / width
 * (with replacement; width*height <= 2^24 keeps the multiply-shift's bias at or below 2^-8 relative).
 * Ray: the pinhole ray rtxn_trace_grid generates for launch pixel (px, py) of a width x height launch with
 * look_at = poses[image] and the set's focal_length / aspect_ratio -- the same function, operation for operation:
 *   u = (float)((2 (px + 0.5) / width - 1) * aspect_ratio), v = (float)(2 (py + 0.5) / height - 1)   (formed in double),
 *   d = normalise(fmaf(-la[2+4k], focal, fmaf(la[4k], u, la[4k+1] v)))_k=0..2,   o_k = la[4k+3] / 10;
 * rays_o gets o, rays_d the normalised d: explicit rays that walk the grid exactly as the pinhole launch's ray does.
 * Target: the `channels` stored values of images[image][py][px]; RTXN_IMAGE_F32 copied, RTXN_IMAGE_U8 (float)v / 255.0f
 * (IEEE division), alpha included.  drawn (optional) records (image, pixel) per ray.
 * Rules (RTXN_ERR_INVALID with a message, before any device is touched): no NULL among images, poses, rays_o, rays_d,
 * targets; n_images >= 1; n_rays >= 1; width, height >= 1 and width*height <= 1 << 24; channels 3 | 4; format F32 | U8. */
enum rtxn_image_format { RTXN_IMAGE_F32 = 0, RTXN_IMAGE_U8 = 1 };
typedef struct rtxn_image_set {
  const void* images;    /* DEVICE: [n_images][height][width][channels], float or uint8_t */
  const float* poses;    /* DEVICE: float[n_images][16], row-major look_at as rtxn_trace_params.look_at */
  int n_images;
  uint32_t width, height;
  int channels;          /* 3 | 4 */
  int format;            /* enum rtxn_image_format */
  float focal_length, aspect_ratio;      /* as rtxn_trace_params */
} rtxn_image_set;
typedef struct rtxn_draw_batch_args {
  rtxn_image_set set;
  int n_rays;
  unsigned seed;
  const int* step;       /* DEVICE int: index of this batch in the sequence; NULL = 0 */
  float* rays_o;         /* float[n_rays][3] */
  float* rays_d;         /* float[n_rays][3] */
  float* targets;        /* float[n_rays][channels] */
  uint32_t* drawn;       /* optional uint32[n_rays][2]: (image, y*width + x) */
} rtxn_draw_batch_args;
int rtxn_draw_batch(const rtxn_draw_batch_args* a, rtxn_stream_t stream);

/* ---- held-out evaluation: PSNR and SSIM of a rendered frame against a resident frame ----------------------
 * Compares pred, a rendered frame float[height*width][3] in the compositor's layout (ray r = pixel (r % width, r / width), so a
 * frame rendered at the set's width x height, focal_length and aspect_ratio lies in the set's own [height][width] order), with
 * frame `image` of an rtxn_image_set, and leaves ONE record of three doubles {mse, psnr, ssim} in device memory.  Two kernels on
 * `stream`, no allocation, no synchronisation, nothing read on the host: hipGraph-capturable behind rtxn_render_frame[_ex].
 * No atomics: a block reduces its tile of the frame to two double partials in the workspace, and one block folds the partials
 * in a fixed order -- the same inputs give the same bits on every run, with and without RTXN_METRICS_SSIM.
 * Target: rtxn_draw_batch's rule (RTXN_IMAGE_F32 copied, RTXN_IMAGE_U8 (float)v / 255.0f); with 4 channels the straight-alpha
 *   pixel over `background`, t_k = fmaf(a, rgb_k, (1.0f - a) * bg_k) = a rgb_k + (1 - a) bg_k in fp32 (a = 1 keeps rgb_k, a = 0
 *   bg_k, exactly).  3 channels: background is not read.
 * RTXN_METRICS_CLAMP: pred is first clamped to [0, 1] (what an 8-bit PNG of the frame keeps); off: pred as it is.
 * mse  = the mean over height*width*3 of (pred - target)^2, differences and squares formed in double;
 * psnr = 10 log10(1 / max(mse, 1e-12))     (120 dB at most; train.psnr()'s rule)
 * ssim (RTXN_METRICS_SSIM; without the flag the slot is NaN): Wang et al. 2004 as mip-NeRF and instant-ngp evaluate it --
 *   an 11 x 11 Gaussian window, sigma = 1.5, normalised to sum 1 and applied separably; K1 = 0.01, K2 = 0.03, L = 1
 *   (C1 = 1e-4, C2 = 9e-4); "valid" windows only, (height - 10)(width - 10) of them, no padding; per channel the weighted
 *   population moments and (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2)); the mean over all windows and
 *   the three channels.  The windowed sums are fp32, taken of each image MINUS a per-tile pivot (that image's own pixel at the
 *   centre of the 16 x 16-window tile, per channel): variances and the covariance are shift-invariant and the means get their
 *   pivot back, so a bright flat region keeps its variance against C2 (the raw-moment form E[x^2] - m^2 loses it in fp32).
 *   The moments and the quotient are formed in double from those sums, each first divided by the squared sum of the eleven
 *   float weights (what rounding them left of 1).
 * Rules (RTXN_ERR_INVALID with a message, before any device is touched): no NULL among set.images, pred, workspace, record
 * (set.poses MAY be NULL: nothing reads it); workspace and record 8-byte aligned; set.n_images >= 1 and 0 <= image < n_images;
 * width, height, channels, format as rtxn_draw_batch; no flag bits beyond the two; with RTXN_METRICS_SSIM width >= 11 and
 * height >= 11; workspace_bytes >= rtxn_image_metrics_workspace_bytes(width, height) (which is 0, with a message, for a frame
 * rtxn_draw_batch would refuse).  The kernels write nothing past that many bytes. */
enum rtxn_metrics_flags { RTXN_METRICS_SSIM = 1, RTXN_METRICS_CLAMP = 2 };
typedef struct rtxn_image_metrics_args {
  rtxn_image_set set;
  int image;             /* which frame of the set: 0 .. n_images - 1 */
  const float* pred;     /* DEVICE float[height*width][3] */
  float background[3];   /* under a 4-channel target */
  int flags;             /* enum rtxn_metrics_flags */
  void* workspace;       /* DEVICE, 8-byte aligned */
  size_t workspace_bytes;
  double* record;        /* DEVICE: 3 doubles {mse, psnr, ssim} */
} rtxn_image_metrics_args;
size_t rtxn_image_metrics_workspace_bytes(uint32_t width, uint32_t height);
int rtxn_image_metrics(const rtxn_image_metrics_args* a, rtxn_stream_t stream);

/* ---- ray gradients through the hash grid, and camera pose refinement ---------------------------------------
 * tiny-cuda-nn's dL/dinput and instant-ngp's extrinsics optimisation.  Three stages, each without atomics and in a fixed order:
 * the same bits on every run, in default and in deterministic mode.  Everything is stream-ordered and hipGraph-capturable.
 *
 * 1. rtxn_hashgrid_input_gradient_segments: dL/d(position), reduced to the segment's end points.  Sample s = 32 j + i sits at
 *    x = fmaf(u, end_j - start_j, start_j), u = i/32 (REGULAR), (i + 0.5)/32 (MIDPOINT_WORLD) or (i + u(seed, step, s))/32
 *    (JITTER_WORLD) -- the forward's own expressions.  Per level l, with fr and the corner indices as the encoder forms them,
 *      d enc_{l,f} / d x_a = (scale_l / 2) sum over the 8 corners c of  sgn_a(c) prod_{b != a} w_b(c) T_l[idx(c)][f],
 *      sgn_a(c) = +1 where bit a of c is set, else -1;  w_b = fr_b or 1 - fr_b
 *    (the exact derivative of the trilinear interpolant inside the cell; a level with scale_l == 0 contributes 0), and
 *      g_s[a]       = sum_{l ascending} sum_{f ascending} (float)dencT[l F + f][s] * d enc_{l,f} / d x_a
 *      dstart[j][a] = k sum_i (1 - u_i) g_s[a],      dend[j][a] = k sum_i u_i g_s[a]          (float[capacity][3] each)
 *    in fp32; the 32-sample sum is a fixed butterfly inside the half wave.  k = unscale (1 / loss_scale), or with scale_device
 *    1 / *scale_device (rtxn_loss_scaler_state::scale, read on the device).  dencT has the row stride the scatter takes it with,
 *    rtxn_padded_samples(32 n_segments).  live_ws (rtxn_live_segments; may be NULL): dencT holds values for the listed segments
 *    only; those are visited, and every unlisted segment of the batch reads back as exact zeros.  jitter may be NULL.
 *    The view-direction columns of dencT are NOT differentiated (instant-ngp's extrinsic gradient does not use them either).
 * 2. rtxn_ray_gradients_reduce: the traversal forms start = fmaf(t_start, d, o), end = fmaf(t_end, d, o), so with the segments
 *    j = indices[r] .. indices[r] + num_stored[r] - 1 of ray r
 *      d_origin[r]    = sum_j (dstart_j + dend_j),      d_direction[r] = sum_j (t_start_j dstart_j + t_end_j dend_j)
 *    (eight lanes per ray, lane q the segments j = q mod 8 in ascending order, then a fixed tree over the lanes; a ray without
 *    segments gets zeros).  These are the partial derivatives with the segment distances and the step lengths HELD FIXED: the
 *    motion of the cell crossings, MIDPOINT_WORLD's step length |end - start| / 32 and which cells are occupied are not
 *    differentiated -- instant-ngp's approximation.  Needs the RTXN_TRACE_DDA distances.
 * 3. rtxn_pose_gradients / rtxn_pose_step: a 6-DoF correction delta = (omega, tau) per image against the untouched poses0,
 *      poses[i] = ( R(omega) R0 | t0 + tau ; poses0's last row ),   R(omega) = I + A K + B K^2,  K = [omega]x,  th = |omega|,
 *      A = sin(th) / th,  B = 2 sin^2(th / 2) / th^2;  below th = 0.25 the Taylor forms through th^8 (truncation < 3e-14).
 *    delta == 0 gives poses[i] == poses0[i] bit for bit.  omega is a LEFT perturbation at the current pose, d' = R(omega) d,
 *    whose gradient is taken at omega = 0 of the current rotation: exact there, first-order accurate beyond (instant-ngp's choice):
 *      g_omega[i] = sum_r rays_d[r] x d_direction[r],   g_tau[i] = sum_r d_origin[r] / 10,   count[i] = number of rays r
 *    over the rays with drawn[r][0] == i (one block per image, each thread its rays in ascending r, then a fixed tree).
 *    rtxn_pose_step, per image: nothing changes when count == 0 (the table's sparse rule), nothing for any image when *skip != 0
 *    (the optimizer guard's skip word, opt->guard + 2), nothing when a gradient component is not finite (that adds one to
 *    *skipped).  Otherwise  steps += 1;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
 *      delta -= lr (m / (1 - b1^steps)) / (sqrt(v / (1 - b2^steps)) + eps)          (1 - b^steps in double, rounded once)
 *    and poses[i] is rewritten from delta.  eps defaults to 1e-15 (tiny-cuda-nn's): pose gradients are of order 1e-6.
 * Rules (RTXN_ERR_INVALID with a message naming the field, before any device is touched): a batch without a hash grid
 * (rtxn_ray_gradients_supported == 0: the lean and frequency paths form no dencT); a NULL among the six buffers of
 * rtxn_ray_gradients; pose without rays; lr < 0, a beta outside [0, 1), eps <= 0, any of them not finite; n_images < 1;
 * RTXN_TRACE_COMPAT in the step.  With a regulariser rays->t_start / t_end must be the regulariser's buffers. */
typedef struct rtxn_ray_gradients {
  float* t_start;        /* DEVICE float[segment_capacity]: written by the step's traversal (as rtxn_train_regularizer's) */
  float* t_end;
  float* dstart;         /* DEVICE float[segment_capacity][3] */
  float* dend;
  float* d_origin;       /* DEVICE float[n_rays][3]: dL/d(rays_o), unscaled */
  float* d_direction;    /* DEVICE float[n_rays][3]: dL/d(rays_d), unscaled */
} rtxn_ray_gradients;
typedef struct rtxn_pose_refinement {
  int n_images;
  const float* poses0;   /* DEVICE float[n][16]: the poses as loaded, never written */
  float* poses;          /* DEVICE float[n][16]: what rtxn_image_set.poses points at, rewritten by the step */
  float* delta;          /* DEVICE float[n][6]: (omega, tau) */
  float* m;              /* DEVICE float[n][6] */
  float* v;              /* DEVICE float[n][6] */
  int* steps;            /* DEVICE int[n]: updates applied per image */
  float* grad;           /* DEVICE float[n][8]: g_omega, g_tau, the ray count, one pad */
  float lr, beta1, beta2, eps;
  const unsigned* skip;  /* optional DEVICE word: != 0 = this step was skipped (rtxn_optimizer_options.guard + 2) */
  unsigned* skipped;     /* optional DEVICE counter of updates refused for a non-finite gradient */
  const uint32_t* drawn; /* DEVICE uint32[n_rays][2] as rtxn_draw_batch records it: read by rtxn_train_step_rays only */
} rtxn_pose_refinement;
int rtxn_ray_gradients_supported(const rtxn_mlp* mlp, const rtxn_hashgrid* grid);
int rtxn_hashgrid_input_gradient_segments(const rtxn_hashgrid* grid, const void* table_fp16, const float* start_points,
                                          const float* end_points, long n_segments, int sample_type, const void* dencT,
                                          const void* live_ws, const rtxn_sample_jitter* jitter, float unscale,
                                          const float* scale_device, float* dstart, float* dend, rtxn_stream_t stream);
int rtxn_ray_gradients_reduce(const int* indices, const int* num_stored, const float* t_start, const float* t_end,
                              const float* dstart, const float* dend, int n_rays, float* d_origin, float* d_direction,
                              rtxn_stream_t stream);
/* The rules above without the device buffers (what a caller checks before it allocates anything). */
int rtxn_pose_refinement_check(const rtxn_pose_refinement* pose);
int rtxn_pose_gradients(const uint32_t* drawn, const float* rays_d, const float* d_origin, const float* d_direction, int n_rays,
                        const rtxn_pose_refinement* pose, rtxn_stream_t stream);
int rtxn_pose_step(const rtxn_pose_refinement* pose, rtxn_stream_t stream);
/* poses[i] from delta[i] and poses0[i] alone, for every image (a loaded checkpoint, a reset): nothing else is read or written. */
int rtxn_pose_compose(const rtxn_pose_refinement* pose, rtxn_stream_t stream);
/* rtxn_train_gradients_scaled with the ray gradients behind the table scatter (stages 1 and 2 over the batch's dencT, live list
 * and samples; k from batch->loss_scale or the scaler's device word); rays == NULL: exactly rtxn_train_gradients_scaled. */
int rtxn_train_gradients_rays(const rtxn_train_batch* batch, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                              const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_loss_scaler* scaler,
                              const rtxn_ray_gradients* rays, rtxn_stream_t stream);
/* rtxn_train_step_ema with the ray gradients and, optionally, the pose refinement: the traversal's write pass stores t_start /
 * t_end into rays' buffers, stages 1 and 2 run right behind the table scatter -- before any counter advances, so a jitter keyed on
 * the optimizer's step sees the forward's value -- and, with pose, rtxn_pose_gradients (over pose->drawn and trace.rays_d) and
 * rtxn_pose_step run behind the optimizer, where they see the guard's skip word.  rays == NULL and pose == NULL: exactly
 * rtxn_train_step_ema. */
int rtxn_train_step_rays(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                         const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                         const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, const rtxn_ray_gradients* rays,
                         const rtxn_pose_refinement* pose, rtxn_stream_t stream);

/* ---- camera models: per-image intrinsics and lens distortion ------------------------------------------------
 * A ray GENERATOR in front of the stages that walk explicit rays (rtxn_trace_params.rays_o / rays_d): COLMAP's, instant-ngp's and
 * nerfstudio's fl_x, fl_y, cx, cy, k1.., p1, p2.  One model per set; one camera for every image (n_cameras == 1) or one per
 * image.  The parameters live in DEVICE memory, twelve floats per camera:
 *   fx, fy, cx, cy (pixels of the width x height frame), k1, k2, k3, k4, p1, p2, 0, 0.
 * The ray of pixel (px, py) of camera c under the row-major pose la, all in fp32, no contraction:
 *   xd = ((float)px + 0.5f - cx) / fx,   yd = ((float)py + 0.5f - cy) / fy
 *       (the pixel centre and the axes of the pinhole launch: +x along pose column 0 with px, +y along column 1 with py);
 *   RTXN_CAMERA_PINHOLE         q = (xd, yd, -1).
 *   RTXN_CAMERA_OPENCV          q = (x, y, -1) with (x, y) the solution of
 *       xd = x (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 x y + p2 (r2 + 2 x^2),
 *       yd = y (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p2 x y + p1 (r2 + 2 y^2),      r2 = x^2 + y^2   (k4 is not read)
 *     by Newton's method on the analytic 2 x 2 Jacobian from (xd, yd): exactly 8 iterations, no data-dependent exit; an
 *     iteration whose determinant is zero or not finite leaves (x, y) as it is.
 *   RTXN_CAMERA_OPENCV_FISHEYE  thd = sqrt(xd^2 + yd^2); th the solution of thd = th (1 + k1 th^2 + k2 th^4 + k3 th^6 + k4 th^8)
 *     by Newton from th = thd, 8 iterations under the same rule (the derivative in the determinant's place);
 *     q = (sin(th) xd / thd, sin(th) yd / thd, -cos(th)); thd < 1e-8: q = (xd, yd, -1).   (p1, p2 are not read)
 *   d = normalise(fmaf(la[4k+2], q2, fmaf(la[4k], q0, la[4k+1] q1)))_k=0..2,   o_k = la[4k+3] / 10   (the pinhole launch's origin).
 * There is no per-ray validity flag: the parameters must be invertible over the frame, which is the caller's to establish
 * (rtx_nerf_amd.api.camera_set checks it on the host).  These calls only read the parameters; rtxn_camera_refinement below optimises them.
 * rtxn_camera_set_check: host only.  RTXN_ERR_INVALID with a message for a NULL set, an unknown model, n_cameras outside
 *   {1, n_images} or NULL params.
 * rtxn_camera_rays: the rays of launch pixels [ray_begin, ray_begin + ray_count) of a width x height frame of camera `camera`
 *   under look_at (DEVICE, 16 floats), written AT THEIR LAUNCH INDEX into rays_o / rays_d, float[width*height][3] each -- the
 *   layout rtxn_trace_params reads explicit rays in.  Elements outside the window are not touched.  One kernel on `stream`, no
 *   allocation, no synchronisation: capturable.  Rules (RTXN_ERR_INVALID, before a device is touched): the set's own (any
 *   n_cameras >= 1), 0 <= camera < n_cameras, no NULL among look_at, rays_o, rays_d, width, height >= 1 and
 *   width*height <= 2^31 - 1, the window inside the frame.  ray_count == 0 does nothing.
 * rtxn_draw_batch_cameras: rtxn_draw_batch with the ray of the drawn pixel taken from the camera set -- the same hash sequence,
 *   so the same (seed, step, r) picks the same (image, pixel) and copies the same target bits; the ray is the one
 *   rtxn_camera_rays writes for that pixel with camera `image` (camera 0 when n_cameras == 1) and look_at = poses[image], bit
 *   for bit.  set.focal_length and set.aspect_ratio are not read.  Rules: rtxn_draw_batch's, then rtxn_camera_set_check's
 *   against set.n_images. */
enum rtxn_camera_model { RTXN_CAMERA_PINHOLE = 0, RTXN_CAMERA_OPENCV = 1, RTXN_CAMERA_OPENCV_FISHEYE = 2 };
enum { RTXN_CAMERA_PARAMS = 12 };
typedef struct rtxn_camera_set {
  int model;             /* enum rtxn_camera_model: one model per set */
  int n_cameras;         /* 1 (shared by every image) or n_images */
  const float* params;   /* DEVICE float[n_cameras][12]: fx, fy, cx, cy (pixels), k1, k2, k3, k4, p1, p2, 0, 0 */
} rtxn_camera_set;
int rtxn_camera_set_check(const rtxn_camera_set* cameras, int n_images);
int rtxn_camera_rays(const rtxn_camera_set* cameras, int camera, const float* look_at, uint32_t width, uint32_t height,
                     uint32_t ray_begin, uint32_t ray_count, float* rays_o, float* rays_d, rtxn_stream_t stream);
int rtxn_draw_batch_cameras(const rtxn_draw_batch_args* a, const rtxn_camera_set* cameras, rtxn_stream_t stream);
/* The serial frame of rtxn_render_frame_ex over the CALLER'S rays instead of a pose: rays_o, rays_d DEVICE
 * float[cfg.width*cfg.height][3], indexed by launch ray (what rtxn_camera_rays writes), so windows and the configured interleave
 * select rays as they do for a pose; cfg.focal_length / aspect_ratio and the slot's pose are not read.  The traversal runs with
 * look_at = NULL and the two pointers; every stage behind it -- the per-ray direction product, the fused kernels, the compositor
 * with depth, opacity and background, early termination, the overflow accounting -- is the pose frame's, and none of them reads
 * the pose.  rays_d must be unit vectors, as for rtxn_trace_grid.  The rays are read on `stream` by both traversal passes: they
 * must stay untouched until the frame has run.  Capturable.  There is no pipelined (_async) form over rays.
 * rtxn_render_count_segments_rays: rtxn_render_count_segments over the same rays (synchronises `stream`). */
int rtxn_render_frame_rays(rtxn_render* r, int slot, const float* rays_o, const float* rays_d, uint32_t ray_begin,
                           uint32_t ray_count, const rtxn_render_outputs* outputs, rtxn_stream_t stream);
int rtxn_render_count_segments_rays(rtxn_render* r, const float* rays_o, const float* rays_d, uint32_t ray_begin,
                                    uint32_t ray_count, long* segments, rtxn_stream_t stream);

/* ---- intrinsics refinement: the camera rows optimised beside the poses --------------------------------------
 * instant-ngp's intrinsics optimisation over the rows of rtxn_camera_set, from the dL/d(rays_d) the ray gradients leave.  No
 * float atomics, every sum in a fixed order: the same bits on every run.  Stream-ordered, no allocation, nothing read on the
 * host: hipGraph-capturable.
 *
 * 1. rtxn_camera_gradients.  For ray r drawn at pixel (px, py) = (pixel % width, pixel / width) of image i (drawn[r] = (i, pixel)),
 *    camera row cam = params[n_cameras == 1 ? 0 : i] and pose rotation R (la = set_poses[i], R_kc = la[4k+c]), the draw formed
 *      xd = (px + 0.5 - cx) / fx,  yd = (py + 0.5 - cy) / fy,  q = U(xd, yd; k),  w = R q,  d = w / |w|
 *    (rtxn_camera_set above) and the kernel forms them again from the live row with the draw's own device functions, so the
 *    point of linearisation is the ray that was drawn.  With g = d_direction[r]:
 *      gw = (g - d (g . d)) / |w|,   gq = R^T gw,   (lx, ly) = dL/d(xd, yd) per model,
 *      dL/dfx = -lx xd / fx,  dL/dfy = -ly yd / fy,  dL/dcx = -lx / fx,  dL/dcy = -ly / fy.
 *    PINHOLE: (lx, ly) = (gq0, gq1); the six distortion entries are exactly 0.
 *    OPENCV: (x, y) = (q0, q1) the Newton solution, r2 = x^2 + y^2, J the symmetric Jacobian of the forward map there (implicit
 *      function theorem):  (lx, ly) = J^-1 (gq0, gq1);  dL/dk_n = -(lx x + ly y) r2^n, n = 1, 2, 3;
 *      dL/dp1 = -(lx 2xy + ly (r2 + 2y^2));  dL/dp2 = -(lx (r2 + 2x^2) + ly 2xy);  dL/dk4 = 0.
 *    OPENCV_FISHEYE: thd = |(xd, yd)|, u = (xd, yd) / thd, th the solution, dpoly = d(th poly(th))/dth there:
 *      gth = cos(th) (gq0 ux + gq1 uy) + sin(th) gq2,  a = sin(th) (gq0, gq1),
 *      (lx, ly) = (gth / dpoly) u + (a - (a . u) u) / thd;  dL/dk_n = -gth th^(2n+1) / dpoly, n = 1..4;  dL/dp1 = dL/dp2 = 0.
 *      thd < 1e-8 (the draw's pinhole branch): the pinhole form for fx..cy, 0 for k.
 *    Two kernels: one thread per ray writes its twelve floats (ten terms, two zeros) into terms[r]; then one block per camera,
 *    thread t summing its camera's rays r = t, t + 256, ... in ascending order, the wave's xor butterfly, the four waves in
 *    order -- rtxn_pose_gradients' fold.  A shared camera (n_cameras == 1) receives every ray.
 *      grad[c] = (dL/dfx, dfy, dcx, dcy, dk1, dk2, dk3, dk4, dp1, dp2, ray count, 0).
 *    drawn[r][0] must be an image of set_poses (what rtxn_draw_batch records); a ray of a camera >= n_cameras is ignored.
 * 2. rtxn_camera_step.  delta[c][10] against the untouched params0, in three groups with a rate and a bound each:
 *      focal       fx = fx0 exp(delta0), fy = fy0 exp(delta1)           gradient of delta: dL/dfx fx, dL/dfy fy (the live fx, fy)
 *      centre      cx = cx0 + delta2, cy = cy0 + delta3  (pixels)       dL/dcx, dL/dcy
 *      distortion  k1..k4, p1, p2 = the loaded values + delta4..9       the entries of grad
 *    An entry is ACTIVE when the model has it (PINHOLE: none of the six; OPENCV: not k4; OPENCV_FISHEYE: not p1, p2) and its
 *    group's rate is > 0.  Per camera: nothing moves when *skip != 0 (rtxn_optimizer_options.guard + 2), when the ray count is
 *    0 (the table's sparse rule) or when no entry is active; a non-finite gradient among the active entries moves nothing for
 *    that camera and adds one to *skipped.  Otherwise steps += 1 and, for every active entry, rtxn_pose_step's Adam with the
 *    group's rate (1 - b^steps in double, rounded once), delta clamped to +- the group's bound, and the entry recomposed into
 *    params.  No word of an inactive entry -- delta, moments, parameter -- is written.  delta == 0 composes the loaded word
 *    itself, so a zero delta gives params0 bit for bit.  The bounds are safety rails, not a guarantee of invertibility over
 *    the frame: that stays the host's float64 check (rtx_nerf_amd Trainer.check_cameras()).
 * 3. rtxn_camera_compose: all twelve words of every row from delta and params0 alone (a loaded checkpoint, a reset).
 * rtxn_camera_refinement_check: host only, the rules without the device buffers.  RTXN_ERR_INVALID with a message naming the
 * field: an unknown model, n_cameras < 1, a rate < 0 or not finite, a bound < 0 or NaN, a beta outside [0, 1), eps <= 0.  The
 * device calls also need the seven state buffers, and rtxn_camera_gradients terms (16-byte aligned) and width >= 1. */
typedef struct rtxn_camera_refinement {
  int model, n_cameras;  /* as the rtxn_camera_set the rows belong to */
  uint32_t width;        /* the frames' width: drawn's pixel is py * width + px */
  float lr_focal, lr_center, lr_distortion;                  /* a rate of 0 freezes the group */
  float max_log_focal, max_center, max_distortion;           /* |delta| <= the group's bound */
  float beta1, beta2, eps;
  const float* params0;  /* DEVICE float[n_cameras][12]: the rows as loaded, never written */
  float* params;         /* DEVICE float[n_cameras][12]: what rtxn_camera_set.params points at, rewritten by the step */
  float* delta;          /* DEVICE float[n_cameras][10] */
  float* m;              /* DEVICE float[n_cameras][10] */
  float* v;              /* DEVICE float[n_cameras][10] */
  int* steps;            /* DEVICE int[n_cameras]: updates applied per camera */
  float* grad;           /* DEVICE float[n_cameras][12]: ten sums, the ray count, one pad */
  float* terms;          /* DEVICE float[n_rays][12], 16-byte aligned: rtxn_camera_gradients' per-ray scratch (48 B per ray) */
  const unsigned* skip;  /* optional DEVICE word: != 0 = this step was skipped (rtxn_optimizer_options.guard + 2) */
  unsigned* skipped;     /* optional DEVICE counter of updates refused for a non-finite gradient */
  const uint32_t* drawn; /* DEVICE uint32[n_rays][2] as rtxn_draw_batch records it: read by rtxn_train_step_cameras only */
  const float* poses;    /* DEVICE float[n_images][16], the set's live poses (rtxn_image_set.poses): likewise */
} rtxn_camera_refinement;
int rtxn_camera_refinement_check(const rtxn_camera_refinement* cameras);
int rtxn_camera_gradients(const uint32_t* drawn, const float* d_direction, int n_rays, const float* set_poses,
                          const rtxn_camera_refinement* cameras, rtxn_stream_t stream);
int rtxn_camera_step(const rtxn_camera_refinement* cameras, rtxn_stream_t stream);
int rtxn_camera_compose(const rtxn_camera_refinement* cameras, rtxn_stream_t stream);
/* rtxn_train_step_rays with the intrinsics refinement.  Behind the optimizer: the pose gradient, the camera gradient (over
 * cameras->drawn, rays->d_direction and cameras->poses), the pose step, the camera step -- both gradients see the rotation and
 * the rows the batch was drawn with.  cameras without rays is refused, as is cameras without drawn or poses; cameras == NULL:
 * exactly rtxn_train_step_rays. */
int rtxn_train_step_cameras(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                            const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                            const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, const rtxn_ray_gradients* rays,
                            const rtxn_pose_refinement* pose, const rtxn_camera_refinement* cameras, rtxn_stream_t stream);

/* ---- depth supervision from per-pixel depth maps (instant-ngp's depth loss, depth-nerfacto) ------------------
 * Per ray r, with w_i, m_i exactly as rtxn_train_regularizer defines them:
 *   D_r = sum_i w_i m_i     the B the regularised compositor carries; NOT divided by A (as in instant-ngp);
 *   z_r                     the ray's depth target, a distance along the normalised ray in world units.
 *   v_r   = z_r > 0 (a finite value; 0, negative, NaN: the ray has no target and the term is 0 for it)
 *   e_r   = D_r - z_r
 *   L_z   = (lambda_z / n_rays) sum_r v_r l(e_r)      l: L2, L1 or Huber of rtxn_train_loss (kind, param), not relative L2
 *   g_D   = loss_scale lambda_z v_r l'(e_r) / n_rays        in fp32, no fp16 hand-off (the rule of k above)
 *   dL/dw_i gains g_D m_i;      S gains g_D D_r             (D_r is homogeneous of degree 1 in w)
 * g_D is formed as k_z l'(e_r) with k_z = loss_scale lambda_z / n_rays, the expression and order of the regulariser's k.
 * m_i stays the stratum midpoint under RTXN_SAMPLING_JITTER_WORLD.  m_i is a constant to the ray gradients, as it is for the
 * distortion term: rtxn_ray_gradients differentiates the samples' positions with the segment distances held fixed, and the
 * dependence of D_r on t_start / t_end through m_i is not differentiated.  The normaliser is n_rays, not the number of rays
 * with a target (the alpha term's rule), so shares of a data-parallel batch add up as the colour loss does.
 * Outputs (each optional): depth[r] = D_r, depth_loss[r] = v_r l(e_r).  The term has no state.
 * Rules (RTXN_ERR_INVALID with a message naming the field, before any device is touched): weight finite and >= 0; kind
 * RTXN_LOSS_L2 | _L1 | _HUBER; HUBER needs a finite param > 0; a weight > 0, or either output, needs target, t_start and t_end,
 * the RTXN_VR_NERF compositor and sample_type RTXN_SAMPLING_MIDPOINT_WORLD or _JITTER_WORLD; a step needs RTXN_TRACE_DDA;
 * t_start / t_end must be the buffers of an active regulariser and of the ray gradients when those are given.  In
 * deterministic mode the scalar is summed in a fixed order behind the compositor; with weight > 0 that sum reads `depth` and
 * `target`, so `depth` must then be given (the rule `distortion` follows).  depth == NULL, or weight 0 with both outputs
 * NULL: exactly the call of the rung below -- the same kernels, the same bits. */
typedef struct rtxn_train_depth {
  float weight;          /* lambda_z >= 0, finite */
  int kind;              /* RTXN_LOSS_L2 | RTXN_LOSS_L1 | RTXN_LOSS_HUBER */
  float param;           /* HUBER: delta */
  const float* target;   /* DEVICE float[n_rays]: z_r (rtxn_depth_targets writes them) */
  const float* t_start;  /* DEVICE float per packed segment slot, as rtxn_train_regularizer's */
  const float* t_end;
  float* depth;          /* optional DEVICE float[n_rays]: D_r */
  float* depth_loss;     /* optional DEVICE float[n_rays]: v_r l(e_r) */
} rtxn_train_depth;
/* rtxn_volrender_scaled_train with the depth term (bg, loss, reg and scaler may be NULL; scaler == NULL: loss_scale by value) */
int rtxn_volrender_depth_train(const float* network_outputs, const float* ray_hit, const int* num_hits, const int* indices,
                               int batch_size, int num_samples_per_hit, const float* target, float loss_scale, float* pixels,
                               void* loss_gradients_half, float* loss_sum, void* radiance_gradients,
                               const rtxn_train_background* bg, const rtxn_train_loss* loss, const rtxn_train_regularizer* reg,
                               const rtxn_loss_scaler* scaler, const rtxn_train_depth* depth, rtxn_stream_t stream);
/* rtxn_train_gradients_rays / rtxn_train_step_cameras with the depth term; depth == NULL: exactly those calls.  The step's
 * write pass stores t_start / t_end into the struct's buffers (batch.segment_capacity floats each). */
int rtxn_train_gradients_depth(const rtxn_train_batch* batch, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                               const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_loss_scaler* scaler,
                               const rtxn_ray_gradients* rays, const rtxn_train_depth* depth, rtxn_stream_t stream);
int rtxn_train_step_depth(const rtxn_train_step_args* args, const rtxn_train_background* bg, const rtxn_sample_jitter* jitter,
                          const rtxn_train_loss* loss, const rtxn_train_regularizer* reg, const rtxn_optimizer_options* opt,
                          const rtxn_loss_scaler* scaler, const rtxn_weight_ema* ema, const rtxn_ray_gradients* rays,
                          const rtxn_pose_refinement* pose, const rtxn_camera_refinement* cameras, const rtxn_train_depth* depth,
                          rtxn_stream_t stream);
/* Depth targets of a drawn batch, ONE kernel on `stream`, no allocation, no synchronisation: hipGraph-capturable behind
 * rtxn_draw_batch[_cameras].  For ray r: (image, pixel) = drawn[r], v = depth[image][pixel], la = poses[image] (the LIVE poses,
 * so a pose refinement is honoured), d = rays_d[r]:
 *   t = (float)v * scale             scale: the maps' unit times the world's 0.1 origin scale, formed once on the host
 *   RTXN_DEPTH_RAY: target[r] = t    (the map holds distances along the ray)
 *   RTXN_DEPTH_Z:   target[r] = t / c,   c = -(d0 la[2] + d1 la[6] + d2 la[10]) / sqrtf(la[2]^2 + la[6]^2 + la[10]^2)
 *                   = d . f with f = -normalise(pose column 2), the axis the pinhole ray's -la[2+4k] * focal term points along
 *                   (sums left to right, no contraction, IEEE division and square root)
 *   v <= 0, a non-finite v, c <= 2^-6 (or NaN), and an (image, pixel) outside the set write 0: no target.
 * It takes rays_d, so it is right for every camera model without knowing them.
 * Rules (RTXN_ERR_INVALID with a message, before any device is touched): no NULL among depth, poses, drawn, rays_d, target;
 * format U16 | F32; kind Z | RAY; scale finite and > 0; n_images >= 1; n_rays >= 1; width, height >= 1 and
 * width*height <= 1 << 24 (rtxn_draw_batch's rules). */
enum rtxn_depth_format { RTXN_DEPTH_U16 = 0, RTXN_DEPTH_F32 = 1 };
enum rtxn_depth_kind { RTXN_DEPTH_Z = 0, RTXN_DEPTH_RAY = 1 };
typedef struct rtxn_depth_targets_args {
  const void* depth;     /* DEVICE: [n_images][height][width], uint16_t or float */
  const float* poses;    /* DEVICE: float[n_images][16], as rtxn_image_set.poses */
  int n_images;
  uint32_t width, height;
  int format;            /* enum rtxn_depth_format */
  int kind;              /* enum rtxn_depth_kind */
  float scale;
  int n_rays;
  const uint32_t* drawn; /* DEVICE uint32[n_rays][2] as rtxn_draw_batch records it */
  const float* rays_d;   /* DEVICE float[n_rays][3], normalised */
  float* target;         /* DEVICE float[n_rays] */
} rtxn_depth_targets_args;
int rtxn_depth_targets(const rtxn_depth_targets_args* a, rtxn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RTXN_H */
