"""Loader for librtxn.so (the HIP implementation behind include/rtxn.h).

torch is imported FIRST so that the HIP runtime torch ships (soname
libamdhip64.so.7) is the one instance both torch and librtxn use: device
pointers of torch tensors are then valid in librtxn's kernels and streams are
shared.  There is no CPU fallback: a missing library is an ImportError-grade
failure, and compute entry points fail with RTXN_ERR_HIP without a GPU.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTXN_LIB_PATH: load an alternative build of the same ABI (kernel A/B experiments in tools/)
LIB_PATH = os.environ.get("RTXN_LIB_PATH") or os.path.join(_HERE, "librtxn.so")

RTXN_OK = 0


class RtxnError(RuntimeError):
    pass


class TraceParams(C.Structure):
    """struct rtxn_trace_params (include/rtxn.h)."""
    _fields_ = [
        ("look_at", C.c_void_p),
        ("focal_length", C.c_float),
        ("aspect_ratio", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("rays_o", C.c_void_p),
        ("rays_d", C.c_void_p),
        ("ray_begin", C.c_uint32),
        ("ray_count", C.c_uint32),
        ("window_chunk", C.c_uint32),
        ("window_stride", C.c_uint32),
        ("grid_res", C.c_int),
        ("occupancy", C.c_void_p),
        ("occupancy_coarse", C.c_void_p),
        ("mode", C.c_int),
        ("ray_origins", C.c_void_p),
        ("viewing_direction", C.c_void_p),
        ("num_hits", C.c_void_p),
        ("intersection_arr_size", C.c_int),
        ("indices", C.c_void_p),
        ("start_points", C.c_void_p),
        ("end_points", C.c_void_p),
        ("t_start", C.c_void_p),
        ("t_end", C.c_void_p),
        ("seg_ray", C.c_void_p),
        ("seg_view", C.c_void_p),
        ("segment_capacity", C.c_long),
        ("seg_first", C.c_void_p),
        ("occupancy_bricks", C.c_void_p),
        ("occupancy_super", C.c_void_p),
        ("num_stored", C.c_void_p),
        ("sub_rays", C.c_int),
        ("sub_hits", C.c_void_p),
    ]


class HashGridConfig(C.Structure):
    """struct rtxn_hashgrid_config (include/rtxn.h)."""
    _fields_ = [("n_levels", C.c_int), ("n_features", C.c_int), ("log2_hashmap_size", C.c_int),
                ("base_resolution", C.c_int), ("per_level_scale", C.c_float)]


class ImageDataset(C.Structure):
    """struct rtxn_image_dataset (include/rtxn.h)."""
    _fields_ = [("n_images", C.c_int), ("image_width", C.c_uint), ("image_height", C.c_uint), ("image_channels", C.c_uint),
                ("focal", C.c_float), ("camera_angle_x", C.c_float), ("images", C.POINTER(C.c_float)),
                ("poses", C.POINTER(C.c_float))]


class MlpConfig(C.Structure):
    """struct rtxn_mlp_config (include/rtxn.h)."""
    _fields_ = [(n, C.c_int) for n in (
        "n_pos_dims", "n_pos_freqs", "n_dir_dims", "n_dir_freqs",
        "n_neurons", "n_hidden_layers", "n_output_dims", "output_activation", "encoding", "n_encoded_features")]


class TrainBatch(C.Structure):
    """struct rtxn_train_batch (include/rtxn.h)."""
    _fields_ = [("mlp", C.c_void_p), ("grid", C.c_void_p), ("n_dir_freqs", C.c_int), ("table_fp16", C.c_void_p),
                ("start_points", C.c_void_p), ("end_points", C.c_void_p), ("seg_view", C.c_void_p),
                ("num_stored", C.c_void_p), ("indices", C.c_void_p), ("total_segments", C.c_void_p),
                ("segment_capacity", C.c_long), ("n_rays", C.c_int), ("sample_type", C.c_int), ("t_scale", C.c_float),
                ("vr_mode", C.c_int), ("targets", C.c_void_p), ("loss_scale", C.c_float),
                ("encT", C.c_void_p), ("dencT", C.c_void_p), ("workspace", C.c_void_p), ("output_half", C.c_void_p),
                ("radiance", C.c_void_p), ("t_vals", C.c_void_p), ("radiance_gradients", C.c_void_p),
                ("pixels", C.c_void_p), ("loss_gradients_half", C.c_void_p), ("loss_sum", C.c_void_p),
                ("dparams", C.c_void_p), ("dtable", C.c_void_p), ("dtable_hashed_half", C.c_void_p), ("live_ws", C.c_void_p),
                ("skip_table_backward", C.c_int), ("workspace_lean", C.c_int)]


class TrainState(C.Structure):
    """struct rtxn_train_state (include/rtxn.h)."""
    _fields_ = [("mlp_master", C.c_void_p), ("mlp_params_fp16", C.c_void_p), ("mlp_m", C.c_void_p), ("mlp_v", C.c_void_p),
                ("table_master", C.c_void_p), ("table_params_fp16", C.c_void_p), ("table_m", C.c_void_p), ("table_v", C.c_void_p),
                ("table_steps", C.c_void_p), ("step", C.c_void_p), ("effective_lr", C.c_void_p),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("table_lr", C.c_float), ("table_eps", C.c_float), ("loss_scale_divisor", C.c_float)]


class TrainStepArgs(C.Structure):
    """struct rtxn_train_step_args (include/rtxn.h)."""
    _fields_ = [("trace", TraceParams), ("scan_workspace", C.c_void_p), ("scan_workspace_bytes", C.c_size_t),
                ("batch", TrainBatch), ("opt", TrainState)]


class TrainBackground(C.Structure):
    """struct rtxn_train_background (include/rtxn.h)."""
    _fields_ = [("mode", C.c_int), ("color", C.c_float * 3), ("seed", C.c_uint), ("step", C.c_void_p), ("target_channels", C.c_int)]


class SampleJitter(C.Structure):
    """struct rtxn_sample_jitter (include/rtxn.h)."""
    _fields_ = [("seed", C.c_uint), ("step", C.c_void_p)]


class TrainLoss(C.Structure):
    """struct rtxn_train_loss (include/rtxn.h)."""
    _fields_ = [("kind", C.c_int), ("param", C.c_float), ("opacity_weight", C.c_float), ("opacity", C.c_void_p)]


class TrainRegularizer(C.Structure):
    """struct rtxn_train_regularizer (include/rtxn.h)."""
    _fields_ = [("distortion_weight", C.c_float), ("t_start", C.c_void_p), ("t_end", C.c_void_p), ("distortion", C.c_void_p),
                ("depth", C.c_void_p)]


class LrSchedule(C.Structure):
    """struct rtxn_lr_schedule (include/rtxn.h)."""
    _fields_ = [("kind", C.c_int), ("warmup_steps", C.c_int), ("decay_start", C.c_int), ("decay_steps", C.c_int), ("ratio", C.c_float),
                ("staircase", C.c_int)]


class OptimizerOptions(C.Structure):
    """struct rtxn_optimizer_options (include/rtxn.h)."""
    _fields_ = [("schedule", LrSchedule), ("weight_decay", C.c_float), ("skip_nonfinite", C.c_int), ("lr_factor", C.c_void_p),
                ("guard", C.c_void_p)]


class GradBuffer(C.Structure):
    """struct rtxn_grad_buffer (include/rtxn.h)."""
    _fields_ = [("data", C.c_void_p), ("count", C.c_long), ("is_fp16", C.c_int)]


class LossScalerState(C.Structure):
    """struct rtxn_loss_scaler_state (include/rtxn.h): the scaler's eight device words."""
    _fields_ = [("scale", C.c_float), ("multiplier", C.c_float), ("good", C.c_int), ("backoffs", C.c_uint), ("growths", C.c_uint),
                ("clipped", C.c_uint), ("grad_norm", C.c_float), ("reserved", C.c_int)]


class LossScaler(C.Structure):
    """struct rtxn_loss_scaler (include/rtxn.h)."""
    _fields_ = [("init_scale", C.c_float), ("growth", C.c_float), ("backoff", C.c_float), ("growth_interval", C.c_int),
                ("min_scale", C.c_float), ("max_scale", C.c_float), ("max_grad_norm", C.c_float), ("state", C.c_void_p),
                ("partials", C.c_void_p)]


class EmaState(C.Structure):
    """struct rtxn_ema_state (include/rtxn.h): the weight EMA's four device words."""
    _fields_ = [("updates", C.c_uint), ("correction", C.c_float), ("reserved", C.c_uint * 2)]


class WeightEma(C.Structure):
    """struct rtxn_weight_ema (include/rtxn.h)."""
    _fields_ = [("decay", C.c_float), ("state", C.c_void_p), ("mlp_ema", C.c_void_p), ("table_ema", C.c_void_p),
                ("table_stamps", C.c_void_p)]


class ImageSet(C.Structure):
    """struct rtxn_image_set (include/rtxn.h)."""
    _fields_ = [("images", C.c_void_p), ("poses", C.c_void_p), ("n_images", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32),
                ("channels", C.c_int), ("format", C.c_int), ("focal_length", C.c_float), ("aspect_ratio", C.c_float)]


class DrawBatchArgs(C.Structure):
    """struct rtxn_draw_batch_args (include/rtxn.h)."""
    _fields_ = [("set", ImageSet), ("n_rays", C.c_int), ("seed", C.c_uint), ("step", C.c_void_p), ("rays_o", C.c_void_p),
                ("rays_d", C.c_void_p), ("targets", C.c_void_p), ("drawn", C.c_void_p)]


class CameraSet(C.Structure):
    """struct rtxn_camera_set (include/rtxn.h)."""
    _fields_ = [("model", C.c_int), ("n_cameras", C.c_int), ("params", C.c_void_p)]


class ImageMetricsArgs(C.Structure):
    """struct rtxn_image_metrics_args (include/rtxn.h)."""
    _fields_ = [("set", ImageSet), ("image", C.c_int), ("pred", C.c_void_p), ("background", C.c_float * 3), ("flags", C.c_int),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("record", C.c_void_p)]


class RayGradients(C.Structure):
    """struct rtxn_ray_gradients (include/rtxn.h)."""
    _fields_ = [("t_start", C.c_void_p), ("t_end", C.c_void_p), ("dstart", C.c_void_p), ("dend", C.c_void_p), ("d_origin", C.c_void_p),
                ("d_direction", C.c_void_p)]


class PoseRefinement(C.Structure):
    """struct rtxn_pose_refinement (include/rtxn.h)."""
    _fields_ = [("n_images", C.c_int), ("poses0", C.c_void_p), ("poses", C.c_void_p), ("delta", C.c_void_p), ("m", C.c_void_p),
                ("v", C.c_void_p), ("steps", C.c_void_p), ("grad", C.c_void_p), ("lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("skip", C.c_void_p), ("skipped", C.c_void_p), ("drawn", C.c_void_p)]


class CameraRefinement(C.Structure):
    """struct rtxn_camera_refinement (include/rtxn.h)."""
    _fields_ = [("model", C.c_int), ("n_cameras", C.c_int), ("width", C.c_uint32), ("lr_focal", C.c_float), ("lr_center", C.c_float),
                ("lr_distortion", C.c_float), ("max_log_focal", C.c_float), ("max_center", C.c_float), ("max_distortion", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("params0", C.c_void_p), ("params", C.c_void_p),
                ("delta", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("steps", C.c_void_p), ("grad", C.c_void_p),
                ("terms", C.c_void_p), ("skip", C.c_void_p), ("skipped", C.c_void_p), ("drawn", C.c_void_p), ("poses", C.c_void_p)]


class TrainDepth(C.Structure):
    """struct rtxn_train_depth (include/rtxn.h)."""
    _fields_ = [("weight", C.c_float), ("kind", C.c_int), ("param", C.c_float), ("target", C.c_void_p), ("t_start", C.c_void_p),
                ("t_end", C.c_void_p), ("depth", C.c_void_p), ("depth_loss", C.c_void_p)]


class DepthTargetsArgs(C.Structure):
    """struct rtxn_depth_targets_args (include/rtxn.h)."""
    _fields_ = [("depth", C.c_void_p), ("poses", C.c_void_p), ("n_images", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32),
                ("format", C.c_int), ("kind", C.c_int), ("scale", C.c_float), ("n_rays", C.c_int), ("drawn", C.c_void_p),
                ("rays_d", C.c_void_p), ("target", C.c_void_p)]


class RenderConfig(C.Structure):
    """struct rtxn_render_config (include/rtxn.h)."""
    _fields_ = [("mlp", C.c_void_p), ("grid", C.c_void_p), ("table_fp16", C.c_void_p), ("n_dir_freqs", C.c_int),
                ("width", C.c_uint32), ("height", C.c_uint32), ("focal_length", C.c_float), ("aspect_ratio", C.c_float),
                ("max_rays", C.c_uint32), ("window_chunk", C.c_uint32), ("window_stride", C.c_uint32), ("grid_res", C.c_int),
                ("occupancy", C.c_void_p), ("trace_mode", C.c_int), ("sub_rays", C.c_int), ("vr_mode", C.c_int),
                ("sample_type", C.c_int), ("step_scale", C.c_float), ("max_segments", C.c_long), ("n_slots", C.c_int),
                ("flags", C.c_int)]


class RenderStats(C.Structure):
    """struct rtxn_render_stats (include/rtxn.h)."""
    _fields_ = [(n, C.c_long) for n in ("frames", "frames_checked", "overflow_frames", "max_segments_needed", "last_segments",
                                        "max_segments")]


class RenderOutputs(C.Structure):
    """struct rtxn_render_outputs (include/rtxn.h)."""
    _fields_ = [("pixels", C.c_void_p), ("depth", C.c_void_p), ("opacity", C.c_void_p), ("background", C.c_float * 3)]


class RenderTermination(C.Structure):
    """struct rtxn_render_termination (include/rtxn.h)."""
    _fields_ = [("min_transmittance", C.c_float), ("first_round_segments", C.c_int), ("n_rounds", C.c_int)]


class RenderTerminationStats(C.Structure):
    """struct rtxn_render_termination_stats (include/rtxn.h)."""
    _fields_ = [(n, C.c_long) for n in ("frames", "last_shaded_segments", "last_total_segments", "shaded_segments",
                                        "total_segments")]


class OccupancyRefreshArgs(C.Structure):
    """struct rtxn_occupancy_refresh_args (include/rtxn.h)."""
    _fields_ = [("mlp", C.c_void_p), ("grid", C.c_void_p), ("n_dir_freqs", C.c_int), ("table_fp16", C.c_void_p),
                ("grid_res", C.c_int), ("density", C.c_void_p), ("decay", C.c_float), ("thickness_scale", C.c_float),
                ("threshold", C.c_float), ("threshold_mode", C.c_int), ("jitter", C.c_int), ("seed", C.c_uint),
                ("step", C.c_void_p), ("occupancy", C.c_void_p), ("coarse", C.c_void_p), ("bricks", C.c_void_p),
                ("super_mip", C.c_void_p), ("occupied", C.c_void_p), ("mean", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("runs_per_pass", C.c_long)]


class DensityLatticeArgs(C.Structure):
    """struct rtxn_density_lattice_args (include/rtxn.h)."""
    _fields_ = [("mlp", C.c_void_p), ("grid", C.c_void_p), ("n_dir_freqs", C.c_int), ("table_fp16", C.c_void_p),
                ("n", C.c_int * 3), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("scale", C.c_float), ("density", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("runs_per_pass", C.c_long)]


class IsosurfaceArgs(C.Structure):
    """struct rtxn_isosurface_args (include/rtxn.h)."""
    _fields_ = [("density", C.c_void_p), ("n", C.c_int * 3), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("iso", C.c_float),
                ("vertices", C.c_void_p), ("normals", C.c_void_p), ("triangles", C.c_void_p), ("max_vertices", C.c_int),
                ("max_triangles", C.c_int), ("counts", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


# every symbol include/rtxn.h declares: name -> (restype, argtypes)
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float
SYMBOLS = {
    "rtxn_version": (_I, []),
    "rtxn_last_error": (C.c_char_p, []),
    "rtxn_trace_grid": (_I, [C.POINTER(TraceParams), _P]),
    "rtxn_build_occupancy_mip": (_I, [_P, _I, _P, _P]),
    "rtxn_occupancy_from_density": (_I, [_P, _F, _I, _P, _P]),
    "rtxn_build_occupancy_bricks": (_I, [_P, _I, _P, _P]),
    "rtxn_scan_workspace_bytes": (C.c_size_t, [_I]),
    "rtxn_scan_hits": (_I, [_P, _P, _P, _I, _P, C.c_size_t, _P]),
    "rtxn_sample": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _P]),
    "rtxn_volrender_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _I, _P]),
    "rtxn_volrender_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P]),
    "rtxn_volrender_l2_train": (_I, [_P, _P, _P, _P, _I, _I, _P, _F, _P, _P, _P, _P, _P]),
    "rtxn_volrender_l2_train_ex": (_I, [_P, _P, _P, _P, _I, _I, _P, _F, _P, _P, _P, _P, C.POINTER(TrainBackground), _P]),
    "rtxn_mlp_create": (_I, [C.POINTER(MlpConfig), C.POINTER(_P)]),
    "rtxn_mlp_destroy": (_I, [_P]),
    "rtxn_mlp_n_params": (_L, [_P]),
    "rtxn_mlp_padded_output_width": (_I, [_P]),
    "rtxn_mlp_set_reserved_cus": (_I, [_P, _I]),
    "rtxn_mlp_mfma_shape": (_I, [_P]),
    "rtxn_mlp_encoded_width": (_I, [_P]),
    "rtxn_mlp_initialize_params": (_I, [_P, C.c_uint64, _P]),
    "rtxn_mlp_set_params": (_I, [_P, _P, _P]),
    "rtxn_mlp_set_params_training": (_I, [_P, _P, _P]),
    "rtxn_mlp_forward": (_I, [_P, _P, _P, _L, _P]),
    "rtxn_mlp_forward_radiance": (_I, [_P, _P, _P, _L, _P]),
    "rtxn_mlp_forward_segments": (_I, [_P, _P, _P, _P, _P, _L, _P, _P, _P]),
    "rtxn_mlp_forward_segments_compact": (_I, [_P, _P, _P, _P, _P, _L, _P, _P]),
    "rtxn_mlp_ray_direction_bias_supported": (_I, [_P]),
    "rtxn_mlp_ray_direction_bias": (_I, [_P, _P, _P, _I, _P, _P]),
    "rtxn_mlp_forward_segments_rays": (_I, [_P, _P, _P, _P, _P, _I, _P, _L, _P, _P, _P]),
    "rtxn_mlp_forward_segments_rays_compact": (_I, [_P, _P, _P, _P, _P, _I, _P, _L, _P, _P]),
    "rtxn_volrender_fwd_compact": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "rtxn_volrender_fwd_compact_nerf": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "rtxn_volrender_fwd_aux": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "rtxn_hashmlp_supported": (_I, [_P, _P, _I]),
    "rtxn_hashmlp_forward_segments": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P]),
    "rtxn_occupancy_refresh_supported": (_I, [_P, _P, _I]),
    "rtxn_occupancy_refresh_workspace_bytes": (C.c_size_t, [_I, _L]),
    "rtxn_occupancy_refresh": (_I, [C.POINTER(OccupancyRefreshArgs), _P]),
    "rtxn_density_lattice_workspace_bytes": (C.c_size_t, [C.POINTER(C.c_int), _L]),
    "rtxn_density_lattice": (_I, [C.POINTER(DensityLatticeArgs), _P]),
    "rtxn_isosurface_workspace_bytes": (C.c_size_t, [C.POINTER(C.c_int)]),
    "rtxn_isosurface": (_I, [C.POINTER(IsosurfaceArgs), _P]),
    "rtxn_render_workspace_bytes": (C.c_size_t, [C.POINTER(RenderConfig)]),
    "rtxn_render_create": (_I, [C.POINTER(RenderConfig), _P, C.c_size_t, C.POINTER(_P)]),
    "rtxn_render_destroy": (_I, [_P]),
    "rtxn_render_set_occupancy": (_I, [_P, _P, _P]),
    "rtxn_render_count_segments": (_I, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(C.c_long), _P]),
    "rtxn_render_frame": (_I, [_P, _I, _P, C.c_uint32, C.c_uint32, _P, _P]),
    "rtxn_render_frame_async": (_I, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, C.POINTER(_P)]),
    "rtxn_render_frame_async_host": (_I, [_P, C.POINTER(C.c_float), C.c_uint32, C.c_uint32, _P, _P, C.POINTER(_P)]),
    "rtxn_render_frame_ex": (_I, [_P, _I, _P, C.c_uint32, C.c_uint32, C.POINTER(RenderOutputs), _P]),
    "rtxn_render_frame_async_ex": (_I, [_P, _P, _I, C.c_uint32, C.c_uint32, C.POINTER(RenderOutputs), _P, C.POINTER(_P)]),
    "rtxn_render_drain": (_I, [_P, _P]),
    "rtxn_render_status": (_I, [_P, _I, C.POINTER(RenderStats)]),
    "rtxn_render_slot_buffers": (_I, [_P, _I] + [C.POINTER(_P)] * 11),
    "rtxn_render_ray_workspace_bytes": (C.c_size_t, [C.POINTER(RenderConfig)]),
    "rtxn_render_set_ray_workspace": (_I, [_P, _P, C.c_size_t]),
    "rtxn_render_ray_buffers": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P)]),
    "rtxn_render_termination_workspace_bytes": (C.c_size_t, [C.POINTER(RenderConfig), C.POINTER(RenderTermination)]),
    "rtxn_render_set_termination": (_I, [_P, C.POINTER(RenderTermination), _P, C.c_size_t]),
    "rtxn_render_termination_status": (_I, [_P, _I, C.POINTER(RenderTerminationStats)]),
    "rtxn_render_termination_buffers": (_I, [_P, _I, C.POINTER(_P)]),
    "rtxn_padded_samples": (_L, [_L]),
    "rtxn_encode_frequency": (_I, [_P, _P, _P, _L, _P]),
    "rtxn_hashgrid_create": (_I, [C.POINTER(HashGridConfig), C.POINTER(_P)]),
    "rtxn_hashgrid_destroy": (_I, [_P]),
    "rtxn_hashgrid_n_params": (_L, [_P]),
    "rtxn_hashgrid_encoded_width": (_I, [_P, _I]),
    "rtxn_hashgrid_level_offset": (_L, [_P, _I]),
    "rtxn_hashgrid_level_is_hashed": (_I, [_P, _I]),
    "rtxn_half2_workspace_bytes": (C.c_size_t, [_L, _L]),
    "rtxn_half2_count_nonzero": (_I, [_P, _L, _L, _P, _P]),
    "rtxn_half2_pack_nonzero": (_I, [_P, _L, _L, _P, C.c_ulonglong, _L, _P, _P, _I, _P]),
    "rtxn_half2_add_pairs": (_I, [_P, _L, _P, _L, _P]),
    "rtxn_convert_f32_to_f16": (_I, [_P, _P, _L, _P]),
    "rtxn_convert_f16_to_f32": (_I, [_P, _P, _L, _P]),
    "rtxn_hashgrid_encode": (_I, [_P, _I, _P, _P, _P, _L, _P]),
    "rtxn_hashgrid_backward": (_I, [_P, _P, _P, _L, _P, _P]),
    "rtxn_hashgrid_backward_mixed": (_I, [_P, _P, _P, _L, _P, _P, _P]),
    "rtxn_encode_frequency_segments": (_I, [_P, _P, _P, _P, _L, _I, _F, _P, _P, _P]),
    "rtxn_hashgrid_encode_segments": (_I, [_P, _I, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P]),
    "rtxn_hashgrid_backward_segments": (_I, [_P, _P, _P, _L, _I, _P, _P, _P, _P]),
    "rtxn_mlp_train_workspace_bytes": (C.c_size_t, [_P, _L]),
    "rtxn_mlp_train_forward": (_I, [_P, _P, _L, _P, _P, _P, _P]),
    "rtxn_mlp_train_backward": (_I, [_P, _P, _P, _P, _L, _P, _P, _P, _P]),
    "rtxn_mlp_train_recompute_supported": (_I, [_P]),
    "rtxn_mlp_train_forward_outputs": (_I, [_P, _P, _L, _P, _P, _P]),
    "rtxn_mlp_train_backward_recompute": (_I, [_P, _P, _P, _P, _L, _P, _P, _P]),
    "rtxn_l2_loss": (_I, [_P, _P, _L, _F, _P, _P, _P, _P]),
    "rtxn_adam_step": (_I, [_L, _P, _P, _P, _P, _P, _I, _F, _F, _F, _F, _F, _P]),
    "rtxn_adam_step_half_grads": (_I, [_L, _P, _P, _P, _P, _P, _I, _F, _F, _F, _F, _F, _P]),
    "rtxn_adam_effective_lr": (_F, [_F, _F, _F, _I]),
    "rtxn_adam_step_captured": (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, _P]),
    "rtxn_adam_step_sparse": (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, _F, _P]),
    "rtxn_deterministic_workspace_bytes": (C.c_size_t, [_L]),
    "rtxn_set_deterministic_workspace": (_I, [_P, _P]),
    "rtxn_mlp_train_lean_supported": (_I, [_P]),
    "rtxn_mlp_train_lean_workspace_bytes": (C.c_size_t, [_P, _L]),
    "rtxn_mlp_train_forward_lean": (_I, [_P, _P, _L, _P, _P, _P, _P]),
    "rtxn_mlp_train_backward_lean": (_I, [_P, _P, _P, _P, _L, _P, _P, _P, _P]),
    "rtxn_mlp_train_forward_lean_fused_supported": (_I, [_P]),
    "rtxn_mlp_train_forward_lean_segments": (_I, [_P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P, _P]),
    "rtxn_mlp_train_backward_lean_segments": (_I, [_P, _P, _P, _P, _L, _I, _P, _P, _P, _P, _P, _P]),
    "rtxn_train_gradients": (_I, [C.POINTER(TrainBatch), _P]),
    "rtxn_train_step": (_I, [C.POINTER(TrainStepArgs), _P]),
    "rtxn_train_gradients_ex": (_I, [C.POINTER(TrainBatch), C.POINTER(TrainBackground), _P]),
    "rtxn_train_step_ex": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), _P]),
    "rtxn_live_segments_workspace_bytes": (C.c_size_t, [_L]),
    "rtxn_live_segments": (_I, [_P, _L, _L, _P, _P]),
    "rtxn_mlp_train_backward_recompute_live": (_I, [_P, _P, _P, _P, _L, _P, _P, _P, _P]),
    "rtxn_mlp_train_backward_live": (_I, [_P, _P, _P, _P, _L, _P, _P, _P, _P, _P]),
    "rtxn_mlp_train_forward_live": (_I, [_P, _P, _L, _P, _P, _P]),
    "rtxn_hashgrid_backward_segments_live": (_I, [_P, _P, _P, _L, _I, _P, _P, _P, _P, _P]),
    "rtxn_sample_ex": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _I, C.POINTER(SampleJitter), _P]),
    "rtxn_encode_frequency_segments_jitter": (_I, [_P, _P, _P, _P, _L, _I, _F, _P, _P, C.POINTER(SampleJitter), _P]),
    "rtxn_hashgrid_encode_segments_jitter": (_I, [_P, _I, _P, _P, _P, _P, _L, _I, _F, _P, _P, C.POINTER(SampleJitter), _P]),
    "rtxn_mlp_train_forward_lean_segments_jitter": (_I, [_P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P, C.POINTER(SampleJitter), _P]),
    "rtxn_mlp_train_backward_lean_segments_jitter": (_I, [_P, _P, _P, _P, _L, _I, _P, _P, _P, _P, _P, C.POINTER(SampleJitter), _P]),
    "rtxn_hashgrid_backward_segments_jitter": (_I, [_P, _P, _P, _L, _I, _P, _P, _P, C.POINTER(SampleJitter), _P]),
    "rtxn_hashgrid_backward_segments_live_jitter": (_I, [_P, _P, _P, _L, _I, _P, _P, _P, _P, C.POINTER(SampleJitter), _P]),
    "rtxn_train_gradients_jitter": (_I, [C.POINTER(TrainBatch), C.POINTER(TrainBackground), C.POINTER(SampleJitter), _P]),
    "rtxn_train_step_jitter": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), _P]),
    "rtxn_volrender_loss_train": (_I, [_P, _P, _P, _P, _I, _I, _P, _F, _P, _P, _P, _P, C.POINTER(TrainBackground), C.POINTER(TrainLoss), _P]),
    "rtxn_loss": (_I, [_P, _P, _L, C.POINTER(TrainLoss), _F, _P, _P, _P, _P]),
    "rtxn_train_gradients_loss": (_I, [C.POINTER(TrainBatch), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss), _P]),
    "rtxn_train_step_loss": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss), _P]),
    "rtxn_volrender_reg_train": (_I, [_P, _P, _P, _P, _I, _I, _P, _F, _P, _P, _P, _P, C.POINTER(TrainBackground), C.POINTER(TrainLoss),
                                      C.POINTER(TrainRegularizer), _P]),
    "rtxn_train_gradients_reg": (_I, [C.POINTER(TrainBatch), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                      C.POINTER(TrainRegularizer), _P]),
    "rtxn_train_step_reg": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                 C.POINTER(TrainRegularizer), _P]),
    "rtxn_lr_schedule_factor": (_F, [C.POINTER(LrSchedule), _I]),
    "rtxn_optimizer_options_check": (_I, [C.POINTER(OptimizerOptions)]),
    "rtxn_optimizer_rate": (_I, [C.POINTER(OptimizerOptions), _P, _I, _F, _F, _F, _F, _P, _P, _P]),
    "rtxn_check_gradients": (_I, [C.POINTER(GradBuffer), _I, _P, _P]),
    "rtxn_adam_step_opt": (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, _F, C.POINTER(OptimizerOptions), _P]),
    "rtxn_adam_step_sparse_opt": (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, _F, C.POINTER(OptimizerOptions), _P]),
    "rtxn_train_step_opt": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                 C.POINTER(TrainRegularizer), C.POINTER(OptimizerOptions), _P]),
    "rtxn_loss_scaler_check": (_I, [C.POINTER(LossScaler)]),
    "rtxn_loss_scaler_workspace_bytes": (C.c_size_t, []),
    "rtxn_loss_scaler_init_state": (_I, [C.POINTER(LossScaler), C.POINTER(LossScalerState)]),
    "rtxn_loss_scaler_advance": (_I, [C.POINTER(LossScaler), C.POINTER(LossScalerState), _I, C.c_double, _F, C.POINTER(LossScalerState)]),
    "rtxn_gradient_statistics": (_I, [C.POINTER(GradBuffer), _I, _P, C.POINTER(LossScaler), _P]),
    "rtxn_loss_scaler_step": (_I, [C.POINTER(OptimizerOptions), C.POINTER(LossScaler), C.POINTER(GradBuffer), _I, _P, _I, _F, _F, _F, _F, _P,
                                   _P, _F, _P]),
    "rtxn_adam_step_scaled": (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, C.POINTER(OptimizerOptions), C.POINTER(LossScaler), _P]),
    "rtxn_adam_step_sparse_scaled": (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, C.POINTER(OptimizerOptions), C.POINTER(LossScaler),
                                          _P]),
    "rtxn_volrender_scaled_train": (_I, [_P, _P, _P, _P, _I, _I, _P, _F, _P, _P, _P, _P, C.POINTER(TrainBackground), C.POINTER(TrainLoss),
                                         C.POINTER(TrainRegularizer), C.POINTER(LossScaler), _P]),
    "rtxn_train_gradients_scaled": (_I, [C.POINTER(TrainBatch), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                         C.POINTER(TrainRegularizer), C.POINTER(LossScaler), _P]),
    "rtxn_train_step_scaled": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                    C.POINTER(TrainRegularizer), C.POINTER(OptimizerOptions), C.POINTER(LossScaler), _P]),
    "rtxn_weight_ema_check": (_I, [C.POINTER(WeightEma)]),
    "rtxn_ema_catch_up": (_F, [_F, _F, C.c_uint, _F]),
    "rtxn_ema_correction": (_F, [_F, C.c_uint]),
    "rtxn_optimizer_rate_ema": (_I, [C.POINTER(OptimizerOptions), C.POINTER(WeightEma), _P, _I, _F, _F, _F, _F, _P, _P, _P]),
    "rtxn_loss_scaler_step_ema": (_I, [C.POINTER(OptimizerOptions), C.POINTER(LossScaler), C.POINTER(WeightEma), C.POINTER(GradBuffer), _I, _P,
                                       _I, _F, _F, _F, _F, _P, _P, _F, _P]),
    "rtxn_adam_step_ema": (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, _F, C.POINTER(OptimizerOptions), C.POINTER(LossScaler),
                                C.POINTER(WeightEma), _P, _P]),
    "rtxn_adam_step_sparse_ema": (_I, [_L, _P, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, _F, C.POINTER(OptimizerOptions), C.POINTER(LossScaler),
                                       C.POINTER(WeightEma), _P, _P, _P]),
    "rtxn_ema_weights": (_I, [_L, _P, _P, _P, _P, _F, _P, _P, _P]),
    "rtxn_train_step_ema": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                 C.POINTER(TrainRegularizer), C.POINTER(OptimizerOptions), C.POINTER(LossScaler), C.POINTER(WeightEma), _P]),
    "rtxn_draw_batch": (_I, [C.POINTER(DrawBatchArgs), _P]),
    "rtxn_image_metrics_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rtxn_image_metrics": (_I, [C.POINTER(ImageMetricsArgs), _P]),
    "rtxn_ray_gradients_supported": (_I, [_P, _P]),
    "rtxn_hashgrid_input_gradient_segments": (_I, [_P, _P, _P, _P, _L, _I, _P, _P, C.POINTER(SampleJitter), _F, _P, _P, _P, _P]),
    "rtxn_ray_gradients_reduce": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "rtxn_pose_refinement_check": (_I, [C.POINTER(PoseRefinement)]),
    "rtxn_pose_gradients": (_I, [_P, _P, _P, _P, _I, C.POINTER(PoseRefinement), _P]),
    "rtxn_pose_step": (_I, [C.POINTER(PoseRefinement), _P]),
    "rtxn_pose_compose": (_I, [C.POINTER(PoseRefinement), _P]),
    "rtxn_train_gradients_rays": (_I, [C.POINTER(TrainBatch), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                       C.POINTER(TrainRegularizer), C.POINTER(LossScaler), C.POINTER(RayGradients), _P]),
    "rtxn_train_step_rays": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                  C.POINTER(TrainRegularizer), C.POINTER(OptimizerOptions), C.POINTER(LossScaler), C.POINTER(WeightEma),
                                  C.POINTER(RayGradients), C.POINTER(PoseRefinement), _P]),
    "rtxn_camera_refinement_check": (_I, [C.POINTER(CameraRefinement)]),
    "rtxn_camera_gradients": (_I, [_P, _P, _I, _P, C.POINTER(CameraRefinement), _P]),
    "rtxn_camera_step": (_I, [C.POINTER(CameraRefinement), _P]),
    "rtxn_camera_compose": (_I, [C.POINTER(CameraRefinement), _P]),
    "rtxn_train_step_cameras": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                     C.POINTER(TrainRegularizer), C.POINTER(OptimizerOptions), C.POINTER(LossScaler), C.POINTER(WeightEma),
                                     C.POINTER(RayGradients), C.POINTER(PoseRefinement), C.POINTER(CameraRefinement), _P]),
    "rtxn_volrender_depth_train": (_I, [_P, _P, _P, _P, _I, _I, _P, _F, _P, _P, _P, _P, C.POINTER(TrainBackground), C.POINTER(TrainLoss),
                                        C.POINTER(TrainRegularizer), C.POINTER(LossScaler), C.POINTER(TrainDepth), _P]),
    "rtxn_train_gradients_depth": (_I, [C.POINTER(TrainBatch), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                        C.POINTER(TrainRegularizer), C.POINTER(LossScaler), C.POINTER(RayGradients), C.POINTER(TrainDepth), _P]),
    "rtxn_train_step_depth": (_I, [C.POINTER(TrainStepArgs), C.POINTER(TrainBackground), C.POINTER(SampleJitter), C.POINTER(TrainLoss),
                                   C.POINTER(TrainRegularizer), C.POINTER(OptimizerOptions), C.POINTER(LossScaler), C.POINTER(WeightEma),
                                   C.POINTER(RayGradients), C.POINTER(PoseRefinement), C.POINTER(CameraRefinement), C.POINTER(TrainDepth), _P]),
    "rtxn_depth_targets": (_I, [C.POINTER(DepthTargetsArgs), _P]),
    "rtxn_camera_set_check": (_I, [C.POINTER(CameraSet), _I]),
    "rtxn_camera_rays": (_I, [C.POINTER(CameraSet), _I, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "rtxn_draw_batch_cameras": (_I, [C.POINTER(DrawBatchArgs), C.POINTER(CameraSet), _P]),
    "rtxn_render_frame_rays": (_I, [_P, _I, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(RenderOutputs), _P]),
    "rtxn_render_count_segments_rays": (_I, [_P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(C.c_long), _P]),
    "rtxn_load_images_json": (_I, [C.c_char_p, C.c_char_p, _I, C.POINTER(ImageDataset)]),
    "rtxn_free_image_dataset": (None, [C.POINTER(ImageDataset)]),
    "rtxn_load_llff": (_I, [C.c_char_p, _I, _I, C.POINTER(ImageDataset), C.POINTER(C.POINTER(C.c_float))]),
    "rtxn_free_llff_bounds": (None, [C.POINTER(C.c_float)]),
    "rtxn_write_png_rgb8": (_I, [C.c_char_p, _P, _I, _I]),
    "rtxn_load_png_gray16": (_I, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_uint16))]),
    "rtxn_free_png_gray16": (None, [C.POINTER(C.c_uint16)]),
}

_lib = None


def lib():
    """The loaded library; raises if it has not been built (python -c
    'import __graft_entry__ as g; g.build()' or `make`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RtxnError(
                f"{LIB_PATH} is missing: build it with `make` (hipcc --offload-arch=gfx950). "
                "rtx_nerf_amd has no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)  # AttributeError if the ABI drifted from the header
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what="librtxn"):
    if rc != RTXN_OK:
        msg = lib().rtxn_last_error()
        raise RtxnError(f"{what} failed with status {rc}: {msg.decode() if msg else '?'}")
