"""ctypes binding of libalive_vc.so (C ABI: include/alive_vc.h).

The product path has no CPU fallback: if the shared library is missing or a
tensor is not on a HIP device, these helpers raise.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ALIVE_VC_LIB", os.path.join(os.path.dirname(_HERE), "libalive_vc.so"))   # override: kernel A/B builds

_lib = None


class AliveConv(C.Structure):
    _fields_ = [
        ("W", C.c_void_p), ("bias", C.c_void_p), ("X", C.c_void_p),
        ("N", C.c_int), ("Ci", C.c_int), ("Tin", C.c_int), ("Co", C.c_int), ("K_pad", C.c_int),
        ("KW", C.c_int), ("stride", C.c_int), ("dil", C.c_int), ("pad_left", C.c_int), ("pad_mode", C.c_int),
        ("Tout", C.c_int), ("up", C.c_int), ("act", C.c_int),
        ("post_add", C.c_void_p), ("ch_scale", C.c_void_p), ("residual", C.c_void_p), ("skip", C.c_void_p),
        ("Y", C.c_void_p), ("Z", C.c_void_p), ("film", C.c_void_p),
        ("film_rows", C.c_int), ("Lf", C.c_int), ("film_scale_row", C.c_int), ("film_shift_row", C.c_int),
        ("precision", C.c_int), ("Ci_pad", C.c_int),
        ("film_t0", C.c_int), ("film_f0", C.c_int), ("film_ld", C.c_int),
        ("Xp", C.c_void_p), ("Zp", C.c_void_p), ("Yp", C.c_void_p), ("yp_planes", C.c_int),
    ]


class AliveGemm(C.Structure):
    _fields_ = [
        ("W", C.c_void_p), ("bias", C.c_void_p), ("P", C.c_void_p),
        ("N", C.c_int), ("T", C.c_int), ("Ci", C.c_int), ("Co", C.c_int), ("planes", C.c_int), ("act", C.c_int),
        ("post_add", C.c_void_p), ("ch_scale", C.c_void_p), ("residual", C.c_void_p),
        ("Y", C.c_void_p), ("Pout", C.c_void_p),
        ("b_plane", C.c_int64), ("b_win", C.c_int64), ("b_row", C.c_int), ("b_cblk", C.c_int), ("b_blk", C.c_int64),
        ("arg_val", C.c_void_p), ("arg_idx", C.c_void_p),
        ("Y2", C.c_void_p), ("y_split", C.c_int),
        ("f16s", C.c_int), ("wscale", C.c_void_p), ("in_unscale", C.c_float), ("pout_scale", C.c_float),
    ]


class AliveRescoreArgs(C.Structure):     # test only (alive_debug_knn_rescore)
    _fields_ = [
        ("cand_val", C.c_void_p), ("cand_idx", C.c_void_p), ("P", C.c_int), ("kp", C.c_int),
        ("s_f32", C.c_void_p), ("rows", C.c_void_p), ("norms", C.c_void_p),
        ("M", C.c_int64), ("frames", C.c_int64), ("Tt", C.c_int64), ("idx_base", C.c_int64), ("k", C.c_int),
        ("out_val", C.c_void_p), ("out_idx", C.c_void_p), ("frame_list", C.c_void_p), ("gate_cnt", C.c_void_p),
        ("gate_lo", C.c_int), ("gate_hi", C.c_int), ("flag_list", C.c_void_p), ("flag_cnt", C.c_void_p),
        ("zsig", C.c_float), ("list_len", C.c_int), ("pre_scale", C.c_float), ("sd_prior", C.c_float),
        ("det_q", C.c_void_p), ("det_lib", C.c_void_p), ("thr_list", C.c_void_p),
        ("collect", C.c_int), ("overflow_slack", C.c_float), ("force_fail", C.c_void_p),
    ]


class AliveKnnSearch(C.Structure):       # alive_knn_search_unit
    _fields_ = [
        ("form", C.c_int), ("N", C.c_int), ("T", C.c_int), ("k", C.c_int),
        ("src", C.c_void_p), ("lib_stage", C.c_void_p), ("lib_bf16", C.c_void_p), ("lib_lo", C.c_void_p),
        ("rows_f32", C.c_void_p), ("norms", C.c_void_p), ("rows_hat", C.c_void_p), ("bound", C.c_void_p),
        ("y", C.c_void_p), ("lib_sub", C.c_void_p), ("rho", C.c_void_p), ("sub_w", C.c_void_p), ("rot_c0", C.c_float),
        ("M", C.c_int64), ("idx_base", C.c_int64),
        ("out_val", C.c_void_p), ("out_idx", C.c_void_p), ("ws", C.c_void_p), ("ev_start", C.c_void_p), ("ev_stop", C.c_void_p),
    ]


KNN_BF16, KNN_STRICT, KNN_FP8, KNN_FP6, KNN_FP8_ROT, KNN_FP6_SUB = range(6)       # AliveKnnSearch.form (include/alive_vc.h)

_VP, _I, _I64, _F, _D, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t

# name -> (restype, argtypes); mirrors include/alive_vc.h one to one
PROTOTYPES = {
    "alive_last_error": (C.c_char_p, []),
    "alive_version": (_I, []),
    "alive_library_padded_rows": (_I64, [_I64]),
    "alive_library_pack": (_I, [_VP, _I64, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_workspace_bytes": (_SZ, [_I64, _I64]),
    "alive_knn_workspace_bytes_strict": (_SZ, [_I64, _I64]),
    "alive_knn_workspace_bytes_fast": (_SZ, [_I64, _I64]),
    "alive_knn_search": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP]),
    "alive_library_fp8_bytes": (_SZ, [_I64]),
    "alive_library_rounding_bound": (_I, [_VP, _VP, _VP, _I64, _VP, _VP]),
    "alive_library_pack_lo": (_I, [_VP, _VP, _VP, _I64, _VP, _VP]),
    "alive_knn_search_strict": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_library_pack_fp8": (_I, [_VP, _I64, _VP, _VP]),
    "alive_knn_search_fp8": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_search_stats": (_VP, [_I, _I, _I64, _VP]),
    "alive_debug_knn_stage_view": (_I, [_I64, _I64, _I, _I, _VP, _I]),
    "alive_debug_knn_sub_stage": (_I, [_VP, _VP, _I64, _VP, _VP, _I64, _I, _VP, _VP, _VP, _VP]),
    "alive_debug_knn_rescore": (_I, [C.POINTER(AliveRescoreArgs), _VP]),                              # test only
    "alive_debug_knn_rescore_pool": (_I, [C.POINTER(AliveRescoreArgs), _VP, _VP, _VP, _VP, _I, _VP]),  # test only
    "alive_debug_knn_pool_fields": (_I, [_VP, _I]),                                                   # test only
    "alive_knn_search_timed": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_knn_search_fp8_timed": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_library_pack_fp6": (_I, [_VP, _I64, _VP, _VP]),
    "alive_knn_sub_coordinates": (_I, []),
    "alive_knn_sub_frames": (_I, [_I]),
    "alive_knn_workspace_bytes_sub": (_SZ, [_I64, _I64]),
    "alive_library_fp6_sub_bytes": (_SZ, [_I64]),
    "alive_library_pack_fp6_sub": (_I, [_VP, _I64, _I64, _I64, _VP, _VP, _VP, _VP]),
    "alive_knn_search_fp6_sub_timed": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_library_pack_unit_rows": (_I, [_VP, _VP, _I64, _VP, _VP]),
    "alive_knn_search_unit": (_I, [C.POINTER(AliveKnnSearch), _VP]),
    "alive_knn_rot_coordinates": (_I, []),
    "alive_knn_rot_leading": (_I, []),
    "alive_knn_rot_mixed": (_I, []),
    "alive_library_pack_fp8_rot": (_I, [_VP, _I64, _I64, _I64, _F, _VP, _VP]),
    "alive_knn_search_fp8_rot_timed": (_I, [_VP, _VP, _F, _I, _I, _VP, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_knn_search_fp6": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_search_fp6_timed": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _I64, _I64, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_library_pack_rows": (_I, [_VP, _I64, _I, _VP, _VP, _VP]),
    "alive_knn_grouped_workspace_bytes": (_SZ, [_I, _I, _I]),
    "alive_knn_search_grouped": (_I, [_VP, _I, _I, _VP, _VP, _I64, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_merge_gather_rows": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_knn_blend_gather_rows": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP]),
    "alive_knn_grouped_k_workspace_bytes": (_SZ, [_I, _I, _I]),
    "alive_knn_search_grouped_k": (_I, [_VP, _I, _I, _VP, _VP, _I64, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_merge_gather_rows_k": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_knn_blend_gather_rows_k": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP]),
    "alive_pool_append": (_I, [_VP, _I64, _I64, _I64, _I, _VP, _VP, _I64, _I64, _VP, _VP]),
    "alive_pool_move_rows": (_I, [_VP, _VP, _I64, _I64, _I64, _I64, _VP]),
    # half pool: the fp32 twins' signatures, the row table as fp16 [P][768]
    "alive_pool_append_f16": (_I, [_VP, _I64, _I64, _I64, _I, _VP, _VP, _I64, _I64, _VP, _VP]),
    "alive_pool_move_rows_f16": (_I, [_VP, _VP, _I64, _I64, _I64, _I64, _VP]),
    "alive_knn_search_grouped_f16": (_I, [_VP, _I, _I, _VP, _VP, _I64, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_search_grouped_k_f16": (_I, [_VP, _I, _I, _VP, _VP, _I64, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_merge_gather_rows_f16": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_knn_merge_gather_rows_k_f16": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_knn_blend_gather_rows_f16": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP]),
    "alive_knn_blend_gather_rows_k_f16": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP]),
    "alive_knn_path_rows_f16": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _I64, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "alive_pool_image_bytes": (_SZ, [_VP, _I, _VP]),
    "alive_pool_pack_images": (_I, [_VP, _VP, _I64, _VP, _VP, _I, _VP, _VP, _VP]),
    "alive_knn_pool_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I64, _I64]),
    "alive_knn_search_pool": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _I, _I64, _VP, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_pool_k_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I64, _I64]),
    "alive_knn_search_pool_k": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _I, _I64, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "alive_knn_pool_stats": (_VP, [_VP]),
    "alive_dedup_pass": (_I, [_VP, _VP, _I64, _I, _D, _VP, _VP, _VP]),
    "alive_knn_merge_gather": (_I, [_VP, _VP, _I, _I, _D, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_conv1d": (_I, [C.POINTER(AliveConv), _VP]),
    "alive_conv1d_tiled": (_I, [C.POINTER(AliveConv), _VP]),   # test only
    "alive_conv_up_launches": (_I, [_I]),                      # test only
    "alive_conv_up_min_blocks": (_I, [_I]),                    # test only
    "alive_decoder_precision": (_I, [_I]),
    "alive_encoder_precision": (_I, [_I]),
    "alive_f16_saturations": (_I, [_I]),
    "alive_f16_saturations_clear": (_I, [_VP]),
    "alive_gelu_film": (_I, [_VP, _I, _I, _I, _VP, _I, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP]),
    "alive_planes_bytes": (_SZ, [_I64, _I, _I]),
    "alive_to_planes": (_I, [_VP, _I, _I, _I, _I, _VP, _VP]),
    "alive_gemm_planes": (_I, [C.POINTER(AliveGemm), _VP]),
    "alive_argmax_merge": (_I, [_VP, _VP, _I, _I64, _VP, _VP]),
    "alive_filter_block_small_weights": (_I, [_I]),
    "alive_filter_block_small": (_I, [_VP, _I, _I, _I, _VP, _VP, _I, _I, _I, _VP, _VP, _VP]),
    "alive_filter_block_small_range": (_I, [_VP, _I, _I, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP]),
    "alive_filter_block_small_up_range": (_I, [_VP, _I, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "alive_filter_block_small_wave_range": (_I, [_VP, _I, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "alive_filter_block64_weights": (_I64, []),
    "alive_filter_block64": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP]),
    "alive_filter_block64_range": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP]),
    "alive_filter_block64_range_fp16": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP]),
    "alive_filter_block256_workspace_bytes": (_I64, [_I, _I]),
    "alive_filter_block256_fp16": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _I64, _VP]),
    "alive_filter_block64s_workspace_bytes": (_I64, [_I, _I]),
    "alive_filter_block64s_fp16": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _I64, _VP]),
    "alive_filter_block64s_fp16_up": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "alive_filter_source_in": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_filter_source_out": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP]),
    "alive_dwconv_norm": (_I, [_VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _I, _I, _I, _F, _VP, _VP]),
    "alive_dwconv_norm_planes": (_I, [_VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _I, _I, _I, _F, _I, _VP, _VP]),
    "alive_dwconv_norm_planes_f16s": (_I, [_VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _I, _I, _I, _F, _F, _VP, _VP]),
    "alive_dwconv_norm_planes_ref": (_I, [_VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _I, _I, _I, _F, _I, _VP, _VP, _F]),   # test only
    "alive_channel_norm": (_I, [_VP, _I, _I, _I, _VP, _VP, _F, _VP, _VP]),
    "alive_argmax_channels": (_I, [_VP, _I, _I, _I, _VP, _VP]),
    "alive_oscillator_workspace_bytes": (_SZ, [_I, _I, _I]),
    "alive_oscillator": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _F, _I, _I, _VP, _VP, _VP, _VP]),
    "alive_oscillator_range": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _F, _I, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "alive_dft_basis_bytes": (_SZ, []),
    "alive_dft_basis": (_I, [_VP, _VP]),
    "alive_spectrogram_workspace_bytes": (_SZ, [_I, _I]),
    "alive_spectrogram": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_resample_taps": (_I, [_I, _I]),
    "alive_resample_length": (_I64, [_I64, _I, _I]),
    "alive_resample_filter": (_I, [_I, _I, _VP, _VP]),
    "alive_resample": (_I, [_VP, _I, _I, _I, _I, _VP, _F, _F, _VP, _I, _VP]),
    "alive_resample_rows": (_I, [_VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _I, _VP]),
    "alive_resample_rows_multi": (_I, [_VP, _I, _I, _VP, _VP, _VP, _I, _VP, _I64, _I, _VP, _VP, _VP, _I, _VP, _VP]),
    "alive_pcm16_to_float": (_I, [_VP, _I64, _VP, _VP]),
    "alive_float_to_pcm16": (_I, [_VP, _I64, _VP, _VP]),
    "alive_weight_count": (_I, [_I]),
    "alive_weight_name": (C.c_char_p, [_I, _I]),
    "alive_front_end_workspace_bytes": (_SZ, [_I, _I]),
    "alive_front_end": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP]),
    "alive_content_encoder_workspace_bytes": (_SZ, [_I, _I]),
    "alive_content_encoder": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_f0_estimate_workspace_bytes": (_SZ, [_I, _I]),
    "alive_f0_estimate": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_f0_logits": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_f0_track_workspace_bytes": (_SZ, [_I, _I, _I]),
    "alive_f0_track_rows": (_I, [_VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_voicing_workspace_bytes": (_SZ, [_I, _I]),
    "alive_voicing_rows": (_I, [_VP, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_knn_path_workspace_bytes": (_SZ, [_I, _I, _I]),
    "alive_knn_path_layout": (_I, [_I, _I, _I, _VP]),
    "alive_knn_path_rows": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _I64, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "alive_decoder_workspace_bytes": (_SZ, [_I, _I]),
    "alive_decoder_forward": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "alive_decoder_forward_range": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP]),
    "alive_pitch_transform": (_I, [_VP, _I, _I, _I, _F, _F, _F, _VP]),
    "alive_pitch_transform_rows": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "alive_pitch_stats_groups": (_I, [_VP, _I, _I, _I, _I, _VP, _I, _VP, _VP]),
    "alive_pitch_shift_groups": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "alive_pitch_follow_rows": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _D, _D, _VP, _VP, _VP]),
    "alive_pitch_stats2_groups": (_I, [_VP, _I, _I, _I, _I, _VP, _I, _VP, _VP]),
    "alive_pitch_range_groups": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP, _D, _VP, _VP, _VP, _VP]),
    "alive_pitch_follow2_rows": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _D, _D, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_pitch_transform_rows_centred": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_gate_rows": (_I, [_VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_gate_apply_rows": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "alive_seam_rows": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP]),
    "alive_limit_rows": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP, _VP]),
    "alive_limit_waves": (_I, [_VP, _VP, _I, _I, _VP, _I, _I, _VP, _VP, _VP]),
    "alive_loudness_workspace_bytes": (_SZ, [_I, _I]),
    "alive_loudness_measure_waves": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _D, _I, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "alive_loudness_apply_waves": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _D, _VP, _VP]),
    "alive_loudness_rows": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "alive_envelope_waves": (_I,[_VP, _VP, _I, _VP, _I, _I, _VP, _VP, _I, _I, _D, _D, _D, _VP, _VP]),
    "alive_postfilter_waves": (_I, [_VP, _VP, _I, _I, _VP, _VP, _I, _I, _I, _VP, _VP, _D, _D, _D, _D, _D, _VP, _VP]),
    "alive_ring_push_rows": (_I, [_VP, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "alive_emit_rows": (_I, [_VP, _I, _I, _VP, _VP, _VP, _VP, _I, _VP]),
    "alive_conceal_rows": (_I, [_VP, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP]),
    "alive_codebook_workspace_bytes": (_SZ, [_I64, _I64]),
    "alive_codebook_update": (_I, [_VP, _I64, _I, _VP, _VP, _I64, _VP, _VP, _VP]),
    "alive_codebook_stats": (_I, [_VP, _VP, _VP, _I64, _VP, _VP, _VP]),
    "alive_world_f0_frames": (_I, [_I, _I, _D]),
    "alive_world_f0_taps_count": (_I, [_I, _D, _D]),
    "alive_world_f0_taps": (_I, [_I, _D, _D, _VP]),
    "alive_world_f0_workspace_bytes": (_SZ, [_I, _I, _I, _D, _D, _D]),
    "alive_world_f0": (_I, [_VP, _I, _I, _I, _D, _D, _D, _VP, _VP, _VP, _SZ, _VP]),
    "alive_world_f0_rows": (_I, [_VP, _I, _I, _I, _D, _D, _D, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "alive_linear_resize": (_I, [_VP, _I, _I, _VP, _I, _VP]),
    "alive_world_f0_stages": (_I, [_VP, _I, _I, _I, _D, _D, _D, _VP, _VP, _VP, _SZ, _I, _VP]),   # test only
    "alive_world_f0_layout": (_I, [_I, _I, _I, _D, _D, _D, _VP, _I]),                            # test only
}


def lib():
    """Load libalive_vc.so (built by `make -C alive-vc_amd/csrc` / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().alive_last_error().decode()
        raise ValueError(f"{what}: {msg}" if what else msg)


def ptr(t):
    """device pointer of a contiguous fp32/int32/bf16 HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libalive_vc operates on HIP device tensors only (got a CPU tensor)")
    if not t.is_contiguous():
        raise RuntimeError("libalive_vc needs contiguous tensors")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Workspace:
    """Grow-only device scratch, one per (purpose, device, stream); never allocates inside a call once it has reached its
    steady-state size (hipGraph friendly).  Keyed by the current stream: window batches that run on side streams
    (module/pipeline.py) get scratch of their own."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes, device):
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf


def weight_names(model):
    L = lib()
    return [L.alive_weight_name(model, i).decode() for i in range(L.alive_weight_count(model))]


class WeightTable:
    """Array of device pointers in the order the .so expects, keeping the tensors alive."""

    def __init__(self, model, packed: dict):
        names = weight_names(model)
        missing = [n for n in names if n not in packed]
        if missing:
            raise KeyError(f"packed weights missing {missing[:4]}...")
        self.tensors = [packed[n] for n in names]
        for n, t in zip(names, self.tensors):
            if t.dtype not in (torch.float32, torch.bfloat16) or not t.is_contiguous() or not t.is_cuda:
                raise RuntimeError(f"packed weight {n} must be a contiguous fp32 / bf16 HIP tensor")
        self.array = (C.c_void_p * len(names))(*[t.data_ptr() for t in self.tensors])
        self.names = names

    def tensor(self, name):
        return self.tensors[self.names.index(name)]
