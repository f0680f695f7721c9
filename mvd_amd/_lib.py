"""ctypes binding of libmvd_hip.so (the C ABI declared in include/mvd_hip.h).

There is NO fallback: if the library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import enum
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MVD_HIP_LIB selects another build of the same library (A/B measurements: tools/build_variant.py)
LIB_PATH = os.environ.get("MVD_HIP_LIB") or os.path.join(HERE, "libmvd_hip.so")

MVD_MAX_LEVELS = 4
MVD_USE_CAMERA, MVD_USE_IMAGE, MVD_REUSE_REF, MVD_KEEP_FEATURES, MVD_SHARE_REF = 1, 2, 4, 8, 16
MVD_DEEPCACHE_REFRESH, MVD_DEEPCACHE_SHALLOW = 32, 64


class MvdError(RuntimeError):
    pass


class DebugFlag(enum.IntFlag):
    """mvd_debug_set_flags switches: mvd_debug_flag_t of include/mvd_hip.h without the MVD_DBG_ prefix (the meanings are there;
    tests/test_cabi_cpu.py keeps the two in step).  0 = the product's behaviour."""
    NO_SM_LN_FOLD = 1
    SM_NO_SPLITK = 2
    NO_SM = 4
    NO_SPLIT_KV = 8
    ONE_STREAM = 16
    SINGLE_STREAM_POLICY = 32
    SIDE_DEFAULT_PRIORITY = 64
    NO_XS = 128
    NO_WS = 256
    WS_SMALL_MAPS = 512
    WS_BLOCK64 = 1024
    WS_NO_SHORTCUT = 2048
    WS_NOT_IN_ENCODER = 4096
    WS_ONLY_IN_ENCODER = 8192
    WS_THEN_TILED = 16384
    WS_CHECK = 32768
    GRAPH_ONE_STREAM = 65536
    PP_ROW_MAJOR = 131072
    NO_DEEP_CONV_SPLIT = 262144
    LATE_FROM_UP1 = 524288
    NO_UP4 = 1048576
    GN_ONE_PASS = 2097152
    FORK_LATE = 4194304
    SKINNY_VECTOR = 8388608


class mvd_config_t(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int), ("out_channels", C.c_int), ("num_levels", C.c_int),
        ("block_out_channels", C.c_int * MVD_MAX_LEVELS), ("num_heads", C.c_int * MVD_MAX_LEVELS),
        ("layers_per_block", C.c_int), ("cross_attention_dim", C.c_int), ("norm_num_groups", C.c_int),
        ("norm_eps", C.c_float), ("cam_output_dim", C.c_int), ("cam_hidden_dim", C.c_int),
        ("simple_cam_encoder", C.c_int), ("cam_modulation_strength", C.c_float),
    ]


class mvd_vae_config_t(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int), ("latent_channels", C.c_int), ("num_levels", C.c_int),
        ("block_out_channels", C.c_int * MVD_MAX_LEVELS), ("layers_per_block", C.c_int), ("norm_num_groups", C.c_int),
        ("norm_eps", C.c_float),
    ]


class mvd_text_config_t(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_int), ("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_layers", C.c_int),
        ("num_heads", C.c_int), ("max_positions", C.c_int), ("layer_norm_eps", C.c_float), ("act", C.c_int),
    ]


class mvd_vision_config_t(C.Structure):
    _fields_ = [
        ("image_size", C.c_int), ("patch_size", C.c_int), ("hidden_size", C.c_int), ("intermediate_size", C.c_int),
        ("num_layers", C.c_int), ("num_heads", C.c_int), ("projection_dim", C.c_int), ("layer_norm_eps", C.c_float), ("act", C.c_int),
    ]


class mvd_forward_args_t(C.Structure):
    _fields_ = [
        ("batch", C.c_int), ("height", C.c_int), ("width", C.c_int), ("text_len", C.c_int),
        ("sample", C.c_void_p), ("timesteps", C.c_void_p), ("text", C.c_void_p),
        ("source_camera", C.c_void_p), ("target_camera", C.c_void_p), ("cam_rows", C.c_int), ("cam_batch", C.c_int),
        ("fourier_proj", C.c_void_p), ("source_latents", C.c_void_p), ("encoder_text", C.c_void_p),
        ("ref_batch", C.c_int), ("flags", C.c_int), ("out", C.c_void_p), ("views", C.c_int),
    ]


_SIGS = {
    "mvd_last_error": (C.c_char_p, []),
    "mvd_engine_create": (C.c_int, [C.POINTER(mvd_config_t), C.POINTER(C.c_void_p)]),
    "mvd_engine_destroy": (C.c_int, [C.c_void_p]),
    "mvd_engine_set_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]),
    "mvd_engine_clear_weights": (C.c_int, [C.c_void_p, C.c_int]),
    "mvd_engine_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_engine_workspace_bytes_args": (C.c_int64, [C.c_void_p, C.POINTER(mvd_forward_args_t)]),
    "mvd_engine_workspace_bytes_objects": (C.c_int64, [C.c_void_p, C.POINTER(mvd_forward_args_t), C.c_int]),
    "mvd_engine_refcache_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_engine_bind_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "mvd_unet_forward": (C.c_int, [C.c_void_p, C.POINTER(mvd_forward_args_t), C.c_void_p]),
    "mvd_unet_forward_objects": (C.c_int, [C.c_void_p, C.POINTER(mvd_forward_args_t), C.c_int, C.c_void_p]),
    "mvd_unet_forward_ragged": (C.c_int, [C.c_void_p, C.POINTER(mvd_forward_args_t), C.POINTER(C.c_int), C.c_int, C.c_void_p]),
    "mvd_engine_workspace_bytes_ragged": (C.c_int64, [C.c_void_p, C.POINTER(mvd_forward_args_t), C.POINTER(C.c_int), C.c_int]),
    "mvd_debug_ragged_tables": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mvd_engine_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "mvd_engine_profile_summary": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mvd_engine_profile_shapes": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "mvd_engine_set_graph": (C.c_int, [C.c_void_p, C.c_int]),
    "mvd_engine_reference_pixels": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "mvd_engine_reference_encode": (C.c_int, [C.c_void_p, C.POINTER(mvd_forward_args_t), C.c_void_p, C.c_void_p]),
    "mvd_engine_reference_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_engine_share_encoder_weights": (C.c_int, [C.c_void_p, C.c_int]),
    "mvd_engine_num_features": (C.c_int, [C.c_void_p]),
    "mvd_engine_feature_shape": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mvd_engine_get_feature": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_engine_encode_cameras": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_engine_apply_modulation": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_engine_get_camera_embedding": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_engine_film_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_engine_time_projection": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_linear": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_linear_ld": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_ln_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p,
                                   C.c_int, C.c_int, C.c_void_p]),
    "mvd_op_linear_xs": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mvd_op_conv3x3_ws": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mvd_op_conv3x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                 C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "mvd_op_attention_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "mvd_op_attention_objects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p]),
    "mvd_op_attention_mapped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), C.c_int, C.c_void_p]),
    "mvd_debug_attention_mapped_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                     C.c_int, C.c_void_p]),
    "mvd_debug_attention_pair_ws_bytes": (C.c_int64, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                                                      C.c_float, C.c_int]),
    "mvd_debug_attention_pair": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                           C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_attention_split_ws_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_op_attention_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_groupnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_layernorm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_refnorm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_refnorm_grouped": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_film": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_conv_in": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_conv_out": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_nchw_to_nhwc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_nhwc_to_nchw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_f32_to_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mvd_op_skinny_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_int, C.c_void_p]),
    "mvd_op_timestep_embedding": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_camera_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_layernorm_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p]),
    "mvd_op_skinny_linear_grouped": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                               C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "mvd_op_film_params": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mvd_op_film_params_grouped": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "mvd_op_im2col_in": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_film_nchw_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_gemm_num_configs": (C.c_int, []),
    "mvd_debug_last_gemm_plan": (C.c_int, [C.POINTER(C.c_int)]),
    "mvd_debug_up4_launches": (C.c_long, []),
    "mvd_op_conv3x3_up4": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_void_p]),
    "mvd_debug_last_gemm_nowait": (C.c_int, []),
    "mvd_debug_last_attention_plan": (C.c_int, [C.POINTER(C.c_int)]),
    "mvd_debug_last_groupnorm_plan": (C.c_int, [C.POINTER(C.c_int)]),
    "mvd_debug_pick_splitk": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_debug_pick_splitk_conv": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "mvd_debug_dense_route": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "mvd_debug_gemm_pp_takes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_gemm_sm_num_tiles": (C.c_int, []),
    "mvd_debug_set_attention_nw": (C.c_int, [C.c_int]),
    "mvd_debug_set_flags": (C.c_int, [C.c_int]),
    "mvd_op_ddpm_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_op_cfg_combine": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_op_sampler_step": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                      C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_op_cfg_rescale": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "mvd_op_sampler_step_rescaled": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                               C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                               C.c_int64, C.c_int64, C.c_void_p]),
    "mvd_debug_cfg_rescale_plan": (C.c_int, [C.c_int64, C.POINTER(C.c_int)]),
    "mvd_op_apg": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int64,
                             C.c_int64, C.c_void_p]),
    "mvd_op_sampler_step_apg": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "mvd_debug_apg_plan": (C.c_int, [C.c_int64, C.POINTER(C.c_int)]),
    "mvd_op_unipc_step": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_engine_set_freeu": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float]),
    "mvd_engine_clear_freeu": (C.c_int, [C.c_void_p]),
    "mvd_engine_set_tome": (C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int]),
    "mvd_engine_clear_tome": (C.c_int, [C.c_void_p]),
    "mvd_engine_tome_table": (C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_tome_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mvd_op_tome_match": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_op_tome_merge": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_tome_unmerge_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_debug_tome_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "mvd_engine_set_taps": (C.c_int, [C.c_void_p, C.c_int]),
    "mvd_engine_num_taps": (C.c_int, [C.c_void_p]),
    "mvd_engine_tap_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]),
    "mvd_engine_get_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_engine_set_todo": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mvd_engine_clear_todo": (C.c_int, [C.c_void_p]),
    "mvd_engine_todo_keys": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "mvd_op_todo_downsample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_engine_set_deepcache": (C.c_int, [C.c_void_p, C.c_int]),
    "mvd_engine_clear_deepcache": (C.c_int, [C.c_void_p]),
    "mvd_engine_deepcache_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mvd_engine_bind_deepcache": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvd_op_freeu": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    "mvd_op_add_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int64, C.c_void_p]),
    "mvd_op_noise_loss_ws_bytes": (C.c_int64, [C.c_int, C.c_int64]),
    "mvd_op_noise_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_void_p]),
    "mvd_op_image_metrics_ws_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_op_image_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_vae_create": (C.c_int, [C.POINTER(mvd_vae_config_t), C.POINTER(C.c_void_p)]),
    "mvd_vae_destroy": (C.c_int, [C.c_void_p]),
    "mvd_vae_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]),
    "mvd_vae_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_vae_bind_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvd_vae_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_vae_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_vae_mid_attention_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_vae_mid_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_softmax_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_gaussian_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "mvd_text_create": (C.c_int, [C.POINTER(mvd_text_config_t), C.POINTER(C.c_void_p)]),
    "mvd_text_destroy": (C.c_int, [C.c_void_p]),
    "mvd_text_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]),
    "mvd_text_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "mvd_text_bind_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvd_text_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_attention_causal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "mvd_vision_create": (C.c_int, [C.POINTER(mvd_vision_config_t), C.POINTER(C.c_void_p)]),
    "mvd_vision_destroy": (C.c_int, [C.c_void_p]),
    "mvd_vision_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]),
    "mvd_vision_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_vision_bind_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvd_vision_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_vision_patch_rows_offset": (C.c_int64, [C.c_void_p]),
    "mvd_vision_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_clip_pool_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_clip_cosine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_text_add_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "mvd_op_vision_add_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "mvd_op_text_act": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_vision_act": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_text_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_vit_patchify": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_vit_embed_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                      C.c_void_p, C.c_void_p]),
    "mvd_op_vit_fold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mvd_op_clip_l2norm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mvd_op_vae_pointwise": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_debug_clip_linear_ws_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_debug_clip_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_int64, C.POINTER(C.c_int), C.c_void_p]),
    "mvd_debug_clip_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mvd_vgg_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "mvd_vgg_destroy": (C.c_int, [C.c_void_p]),
    "mvd_vgg_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]),
    "mvd_vgg_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mvd_vgg_bind_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvd_vgg_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "mvd_vgg_perceptual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_conv3x3_relu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_linear_relu": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_maxpool2x2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_sqdiff_mean_ws_bytes": (C.c_int64, [C.c_int, C.c_int64]),
    "mvd_op_sqdiff_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_lpips_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "mvd_lpips_destroy": (C.c_int, [C.c_void_p]),
    "mvd_lpips_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]),
    "mvd_lpips_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mvd_lpips_bind_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvd_lpips_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "mvd_lpips_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "mvd_op_im2col_patch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p,
                                      C.c_void_p]),
    "mvd_op_maxpool3x3s2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_lpips_head_ws_bytes": (C.c_int64, [C.c_int, C.POINTER(C.c_int), C.c_int]),
    "mvd_op_lpips_head": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_fid_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_void_p)]),
    "mvd_fid_destroy": (C.c_int, [C.c_void_p]),
    "mvd_fid_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]),
    "mvd_fid_feature_dim": (C.c_int, [C.c_void_p]),
    "mvd_fid_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int]),
    "mvd_fid_bind_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "mvd_fid_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_fid_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_conv_relu_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mvd_op_pool3x3_slice": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                       C.c_void_p]),
    "mvd_op_resize_tf1": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_global_mean": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_feature_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_kid_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "mvd_op_kid_mmd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_fc_logits": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mvd_op_inception_score_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mvd_op_inception_score": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int),
                                         C.c_void_p]),
    "mvd_op_knn_radii_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mvd_op_knn_radii": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mvd_op_manifold_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mvd_op_image_frontend_spans": (C.c_int, [C.POINTER(C.c_int)]),
    "mvd_op_image_frontend_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mvd_op_image_frontend": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

_lib = None


def lib() -> C.CDLL:
    """Load libmvd_hip.so (once).  Raises if it has not been built -- no CPU fallback exists."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MvdError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or python mvd_amd/_build.py)")
        # torch first: it ships its own libamdhip64 and must be the HIP runtime of the process -- if this library (linked
        # against /opt/rocm's copy) were loaded before torch, two runtimes would coexist and every launch on torch's
        # device pointers would fail ("no ROCm-capable device")
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def last_error() -> str:
    return lib().mvd_last_error().decode()


def check(rc: int, what: str = "") -> int:
    if rc is None or rc < 0 or (rc != 0 and what.startswith("!")):
        raise MvdError(f"{what.lstrip('!')}: rc={rc}: {last_error()}")
    return rc


def call(name: str, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise MvdError(f"{name} failed (rc={rc}): {last_error()}")
    return rc


def stream() -> C.c_void_p:
    """the current torch stream, as the ``void* stream`` argument of the entry points"""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(t) -> int:
    """the ``dtype`` argument of the ``*_set_weight`` entry points: 0 fp32, 1 bf16"""
    import torch
    return {torch.float32: 0, torch.bfloat16: 1}[t.dtype]


class Handle:
    """One ``mvd_<family>_t`` (vae, text, vision, vgg, lpips, fid) with its workspace: ``.h`` from ``mvd_<family>_create(*create_args,
    &h)``, destroyed with the object; ``.ws`` grown on demand and bound when it moves (``rebind_always``: on every ``workspace``
    call -- the text tower and the VAE, whose callers may have bound another buffer in between)."""

    def __init__(self, family: str, *create_args, rebind_always: bool = False):
        self.family, self.rebind_always = family, rebind_always
        self.h = C.c_void_p()
        self.ws = None
        call(f"mvd_{family}_create", *create_args, C.byref(self.h))

    def __del__(self):
        try:
            if self.h:
                getattr(lib(), f"mvd_{self.family}_destroy")(self.h)
        except Exception:
            pass

    def set_weights(self, packed) -> None:
        """registers every tensor of ``packed`` ({slot: fp32 / bf16 device tensor}); the caller keeps them alive"""
        for slot, t in packed.items():
            call(f"mvd_{self.family}_set_weight", self.h, slot.encode(), C.c_void_p(t.data_ptr()), t.numel(), dtype_code(t))

    def workspace_bytes(self, *size_args, sizer: str = "workspace_bytes") -> int:
        need = getattr(lib(), f"mvd_{self.family}_{sizer}")(self.h, *size_args)
        if need < 0:
            raise MvdError(f"{self.family} {sizer}: {last_error()}")
        return need

    def workspace(self, device, *size_args, sizer: str = "workspace_bytes") -> None:
        import torch
        need = self.workspace_bytes(*size_args, sizer=sizer)
        moved = self.ws is None or self.ws.numel() < need or self.ws.device != device
        if moved:
            self.ws = None
            self.ws = torch.empty(need, dtype=torch.uint8, device=device)
        if moved or self.rebind_always:
            call(f"mvd_{self.family}_bind_workspace", self.h, C.c_void_p(self.ws.data_ptr()), self.ws.numel())
