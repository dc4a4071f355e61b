"""ctypes binding of librtfs_amd.so (the C ABI declared in include/rtfs_amd.h).

There is no fallback: if the shared library is missing the import of any hot-path module raises,
and every call checks that its tensors live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librtfs_amd.so")

PACK_ENCODER, PACK_AUDIO_BN, PACK_BLOCK, PACK_DUALPATH, PACK_ATTENTION, PACK_TFAR, PACK_CAF, PACK_S3, PACK_DECODER, PACK_BLOCK_LSTM, PACK_DUALPATH_LSTM = range(11)

_ERR = {-1: "bad shape", -2: "workspace too small", -3: "kernel launch failure", -4: "bad argument"}

_p, _i, _z = C.c_void_p, C.c_int, C.c_size_t
# name -> (restype, argtypes); must list every symbol of include/rtfs_amd.h
SIGNATURES = {
    "rtfs_version": (C.c_char_p, []),
    "rtfs_pack_floats": (_z, [_i]),
    "rtfs_num_frames": (_i, [_i]),
    "rtfs_stft_encoder_workspace_bytes": (_z, [_i, _i]),
    "rtfs_stft_encoder_f32": (_i, [_p, _p, _p, _p, _i, _i, _p, _z, _p]),
    "rtfs_audio_bottleneck_workspace_bytes": (_z, [_i]),
    "rtfs_audio_bottleneck_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_block_workspace_bytes": (_z, [_i, _i, _i]),
    "rtfs_block_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _i]),
    "rtfs_dualpath_workspace_bytes": (_z, [_i, _i, _i]),
    "rtfs_dualpath_sru_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _z, _p]),
    "rtfs_dualpath_lstm_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _z, _p]),
    "rtfs_tf_attention_workspace_bytes": (_z, [_i, _i]),
    "rtfs_tf_attention_f32": (_i, [_p, _p, _p, _i, _i, _p, _z, _p]),
    "rtfs_tfar_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "rtfs_tfar_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _z, _p]),
    "rtfs_caf_workspace_bytes": (_z, [_i, _i]),
    "rtfs_caf_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _z, _p]),
    "rtfs_vp_pack_floats": (_z, []),
    "rtfs_vp_block_f32": (_i, [_p, _p, _p, _i, _i, _p]),
    "rtfs_s3_mask_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "rtfs_istft_decoder_workspace_bytes": (_z, [_i, _i]),
    "rtfs_istft_decoder_f32": (_i, [_p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_separator_workspace_bytes": (_z, [_i, _i, _i]),
    "rtfs_set_batch_split": (_i, [_i]),
    "rtfs_set_dw_two_pass": (_i, [_i]),
    "rtfs_debug_launch_count": (C.c_ulonglong, []),
    "rtfs_separator_workspace_bytes_ex": (_z, [_i, _i, _i, _i]),
    "rtfs_separator_forward_ex_f32": (_i, [_p] * 9 + [_i, _i, _i, _i, _p, _z, _p, _p, _i, _i]),
    "rtfs_separator_forward_f32": (_i, [_p] * 9 + [_i, _i, _i, _i, _p, _z, _p, _p, _i]),
    "rtfs_separator_speakers_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "rtfs_separator_speakers_f32": (_i, [_p] * 9 + [_i, _i, _i, _i, _i, _p, _z, _p, _p, _i, _i]),
    "rtfs_separator_targets_workspace_bytes": (_z, [_p, _i, _i, _i, _i]),
    "rtfs_separator_targets_f32": (_i, [_p] * 11 + [_i, _i, _i, _i, _i, _p, _z, _p, _p, _i, _i]),
    "rtfs_sru_workspace_bytes": (_z, [_i, _i]),
    "rtfs_sru_f32": (_i, [_p, _p, _p, _i, _i, _p, _z, _p]),
    "rtfs_sru_train_pack_floats": (_z, []),
    "rtfs_sru_grad_floats": (_z, []),
    "rtfs_sru_saved_floats": (_z, [_i, _i]),
    "rtfs_sru_backward_workspace_bytes": (_z, [_i, _i]),
    "rtfs_sru_forward_train_f32": (_i, [_p, _p, _p, _p, _i, _i, _p]),
    "rtfs_sru_backward_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _p, _z, _p]),
    # DualPathRNN, training side: the same six symbols for each cell (SRU, LSTM, GRU)
    **{f"rtfs_dualpath_{infix}{name}": sig for infix in ("", "lstm_", "gru_") for name, sig in (
        ("train_pack_floats", (_z, [])),
        ("grad_floats", (_z, [])),
        ("saved_floats", (_z, [_i, _i, _i, _i])),
        ("train_workspace_bytes", (_z, [_i, _i, _i, _i])),
        ("forward_train_f32", (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _z, _p])),
        ("backward_f32", (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _z, _p])))},
    "rtfs_cna_param_floats": (_z, [_p]),
    "rtfs_cna_grad_floats": (_z, [_p]),
    "rtfs_cna_saved_floats": (_z, [_p, _i, _i, _i]),
    "rtfs_cna_workspace_bytes": (_z, [_p, _i, _i, _i]),
    "rtfs_cna_saved_stats_offset": (_z, [_p, _i, _i, _i]),
    "rtfs_cna_grad_norm_offsets": (None, [_p, _p, _p]),
    "rtfs_cna_out_shape": (None, [_p, _i, _i, _p, _p]),
    "rtfs_cna_forward_train_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_cna_bn_update_f32": (_i, [_p, _p, _i, _i, _i, _p, _p, C.c_float, _p]),
    "rtfs_cna_backward_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_tf_attention_train_pack_floats": (_z, []),
    "rtfs_tf_attention_grad_floats": (_z, []),
    "rtfs_tf_attention_saved_floats": (_z, [_i, _i]),
    "rtfs_tf_attention_train_workspace_bytes": (_z, [_i, _i]),
    "rtfs_tf_attention_forward_train_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_tf_attention_backward_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_layout_f32": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "rtfs_adaptive_avg_pool2d_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_adaptive_avg_pool2d_backward_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_tfar_combine_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_tfar_combine_backward_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_stft_encoder_backward_workspace_bytes": (_z, [_i, _i]),
    "rtfs_stft_encoder_backward_f32": (_i, [_p, _p, _p, _i, _i, _p, _z, _p]),
    "rtfs_istft_decoder_backward_workspace_bytes": (_z, [_i, _i]),
    "rtfs_istft_decoder_backward_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_s3_cmul_f32": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "rtfs_caf_attention_f32": (_i, [_p, _p, _i, _i, _i, _p]),
    "rtfs_caf_attention_backward_f32": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "rtfs_caf_combine_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_caf_combine_backward_f32": (_i, [_p] * 9 + [_i, _i, _i, _i, _p]),
    "rtfs_caf_combine_rows_f32": (_i, [_p] * 5 + [_i] * 5 + [_p]),
    "rtfs_caf_combine_rows_backward_f32": (_i, [_p] * 9 + [_i] * 5 + [_p]),
    "rtfs_gateway_grad_floats": (_z, [_i]),
    "rtfs_gateway_workspace_bytes": (_z, [_i]),
    "rtfs_gateway_forward_train_f32": (_i, [_p] * 6 + [_z, _i, _p]),
    "rtfs_gateway_backward_f32": (_i, [_p] * 8 + [_z, _i, _p, _z, _p]),
    "rtfs_pit_sdr_backward_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_layernorm_rows_f32": (_i, [_p, _p, _p, _p, _i, _i, _p]),
    "rtfs_layernorm_rows_backward_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _p]),
    "rtfs_linear_rows_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "rtfs_linear_rows_backward_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_mha_core_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_mha_core_backward_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_debug_gemm_f32": (_i, [_i, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_debug_dw_f32": (_i, [_i, _p, _i, _p, _i, _p, _i, _p, _i, _p]),
    "rtfs_debug_pw_f32": (_i, [_i, _p, _i, _p, _i, _p, _i, _p, _i, _p]),
    "rtfs_debug_attn_f32": (_i, [_i, _p, _i, _p, _i, _p, _i, _p, _i, _p]),
    "rtfs_debug_attn_vscale": (C.c_double, []),
    "rtfs_debug_sweep_stamps": (_i, [_p, _p, _p, _i, _i, _i, _p, _p]),
    "rtfs_selftest_mfma_f16": (_i, [_p, _p, _p, _p]),
    "rtfs_selftest_nearest_index": (_i, [_p, _i, _p, _p, _p, _p]),
    "rtfs_sweep_timing_enable": (_i, [_i]),
    "rtfs_sweep_timing_collect": (_i, [_p, _p, _p, _i]),
    "rtfs_pit_pairwise_sdr_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "rtfs_stoi_workspace_bytes": (_z, [_i, _i, _i]),
    "rtfs_stoi_f32": (_i, [_p, _p, _i, _i, _i, _p, _z, _p, _p, _p]),
    "rtfs_score_many_plan": (_i, [_p, _i, _i, _i, _p, C.POINTER(C.c_size_t)]),
    "rtfs_stoi_many_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p]),
    "rtfs_sdr_many_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p]),
    "rtfs_estoi_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "rtfs_estoi_f32": (_i, [_p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _p]),
    "rtfs_estoi_many_workspace_bytes": (_z, [_p, _i, _i]),
    "rtfs_estoi_many_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _p]),
    "rtfs_bss_sdr_workspace_bytes": (_z, [_i, _i, _i, _i]),
    "rtfs_bss_sdr_f32": (_i, [_p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _p]),
    "rtfs_bss_sdr_many_workspace_bytes": (_z, [_p, _i, _i]),
    "rtfs_bss_sdr_many_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _p]),
    "rtfs_debug_bss_f64": (_i, [_p, _p, _p, _i, _i, _i, _p, _z, _p, _p, _p, _i, _p, _p, _p, _p, _p]),
    "rtfs_bss_eval_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "rtfs_bss_eval_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _z, _p, _p, _p, _p, _p, _i, _p]),
    "rtfs_bss_eval_many_workspace_bytes": (_z, [_p, _i, _i, _i]),
    "rtfs_bss_eval_many_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _z, _p, _p, _p, _p, _p, _i, _p]),
    "rtfs_debug_bss_eval_f64": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _z, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p]),
    "rtfs_longform_plan": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int)]),
    "rtfs_longform_frame_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rtfs_longform_frame_speakers_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_longform_overlap_add_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "rtfs_longform_many_plan": (_i, [_p, _p, _i, _i, _i, _i, _p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "rtfs_longform_frame_many_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_longform_overlap_add_many_f32": (_i, [_p, _p, _p, _i, _i, C.c_longlong, _i, _i, _i, _p]),
    "rtfs_longform_many_speakers_plan": (_i, [_p, _p, _p, _i, _i, _i, _p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "rtfs_longform_frame_many_speakers_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rtfs_longform_overlap_add_many_speakers_f32": (_i, [_p, _p, _p, _i, _i, C.c_longlong, _i, _i, _p]),
    "rtfs_live_plan": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "rtfs_live_ingest_frame_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_live_overlap_add_f32": (_i, [_p, _p, _p, _p, _i, C.c_longlong, _i, _i, _i, _i, _i, _p]),
    "rtfs_live_reset_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_live_speakers_sizes_ok": (_i, [_i, _i, _i, _i]),
    "rtfs_live_ingest_frame_speakers_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_live_reset_speakers_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_live_faces_plan": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _i, _p, _p, _p, _p, _p]),
    "rtfs_live_ingest_frame_faces_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_live_overlap_add_faces_f32": (_i, [_p, _p, _p, _p, _i, C.c_longlong, _i, _i, _i, _i, _i, _p]),
    "rtfs_video_pack_floats": (_z, []),
    "rtfs_video_workspace_bytes": (_z, [_i, _i]),
    "rtfs_video_frontend_f32": (_i, [_p, _p, _p, _i, _i, _p, _z, _p]),
    "rtfs_live_video_plan": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "rtfs_live_video_ingest_u8": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, C.c_double, C.c_double, _p]),
    "rtfs_live_video_ingest_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_video_windows_workspace_bytes": (_z, [_i]),
    "rtfs_video_frontend_windows_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _z, _p]),
    "rtfs_live_video_reset": (_i, [_p, _p, _i, _p]),
    "rtfs_frame_rate_map": (_i, [_i, _i, C.c_longlong, _p, _p]),
    "rtfs_live_video_rate_plan": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "rtfs_live_video_ingest_rate_u8": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, C.c_double, C.c_double, _i, _i, _p]),
    "rtfs_live_video_ingest_rate_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "rtfs_lips_prepare_rate_u8": (_i, [_p, _p, _p, _i, _i, _i, _i, C.c_double, C.c_double, _i, _i, _p]),
    "rtfs_timestamp_map": (_i, [_p, C.c_longlong, C.c_longlong, C.c_longlong, _p, _p]),
    "rtfs_live_video_stamp_plan": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, C.c_longlong, _p, _p, _p, _p, _p]),
    "rtfs_live_video_ingest_stamp_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_double, C.c_double, C.c_longlong, _p]),
    "rtfs_live_video_ingest_stamp_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, C.c_longlong, _p]),
    "rtfs_live_video_stamp_reset": (_i, [_p, _p, _p, _i, _p]),
    "rtfs_optim_plan": (_i, [_p, _i, _p, _p, _p]),
    "rtfs_optim_gather_f32": (_i, [_p, _p, _i, _i, _p, _p, _i, _p]),
    "rtfs_optim_sumsq_f32": (_i, [_p, _i, _i, _p, _p, _p]),
    "rtfs_optim_adamw_f32": (_i, [_p, _p, _p, _i, _p, _i, _i, _p, _p, _p, _p, C.c_float, C.c_float, _p, _p]),
    "rtfs_lips_prepare_u8": (_i, [_p, _p, _p, _i, _i, _i, _i, C.c_double, C.c_double, _p]),
    "rtfs_wav_normalize_workspace_bytes": (_z, [_i, _i, _i]),
    "rtfs_wav_normalize_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, C.c_double, _p, _z, _p]),
    "rtfs_resample_plan": (_i, [_i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _p]),
    "rtfs_resample_out_len": (C.c_longlong, [_i, _i, C.c_longlong]),
    "rtfs_resample_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "rtfs_mouth_affine": (_i, [_p, _p, C.c_longlong, _i, _i, _i, _i, _p, C.POINTER(C.c_longlong)]),
    "rtfs_mouth_rois_u8": (_i, [_p, _p, _i, _i, _i, _p]),
    "rtfs_live_resample_plan": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, C.c_longlong, _p, _p, _p, _p]),
    "rtfs_live_resample_f32": (_i, [_p, _p, _p, _p, _i, C.c_longlong, C.c_longlong, _i, _i, _i, _p]),
    "rtfs_live_resample_i16": (_i, [_p, _p, _p, _p, _i, C.c_longlong, C.c_longlong, _i, _i, _i, _p]),
    "rtfs_live_resample_reset": (_i, [_p, _p, _i, _i, _i, _p]),
    "rtfs_mix_workspace_bytes": (_z, [_i, _i]),
    "rtfs_mix_plan": (_i, [_p, _p, _i, _i, _i, _p, C.POINTER(C.c_size_t), _p]),
    "rtfs_mix_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, C.c_double, _p, _z, _p]),
    "rtfs_reverb_plan": (_i, [_p, _i, _i, _p, _p]),
    "rtfs_reverb_f32": (_i, [_p, _p, _i, _i, _p]),
    "rtfs_mix_reverb_plan": (_i, [_p, _p, _p, _i, _i, _i, C.c_longlong, _p, C.POINTER(_i), C.POINTER(C.c_size_t), _p]),
    "rtfs_mix_reverb_f32": (_i, [_p, _i, _p, _p, _p, _p, _i, _i, _i, _i, C.c_double, _p, _z, _p]),
    "rtfs_loudness_design": (_i, [_i, _p]),
    "rtfs_loudness_plan": (_i, [_p, _i, _i, _p, C.POINTER(C.c_size_t), _p, _p]),
    "rtfs_loudness_f32": (_i, [_p, _p, _p, _p, _p, _z, _p]),
    "rtfs_loudness_gain_f32": (_i, [_p, _p, _p, C.c_double, _p, _p, _p]),
}

_lib = None


def load():
    """Load librtfs_amd.so once; raise (never fall back) when it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `make -C rtfs-net_amd/csrc` (or __graft_entry__.build()); "
            "the RTFS-Net MI355X path has no non-HIP fallback"
        )
    lib = C.CDLL(LIB_PATH)
    import functools
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
        # size queries are pure functions of a few integers and a training step asks ~1000 of them: memoise (an instance attribute
        # shadows the CDLL's own lookup)
        if res is _z and args and all(a in (_i, _z) for a in args):
            setattr(lib, name, functools.lru_cache(maxsize=None)(fn))
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        _guards().clear()
        raise RuntimeError(f"{what} failed: {_ERR.get(code, code)}")
    if _POISON is not None:
        _check_guards(what)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t: torch.Tensor):
    """torch's current stream on the tensor's device as the void* the C ABI takes (the raw-handle query when this torch has it: building a
    torch.cuda.Stream object per call costs microseconds, ~800 times a step)."""
    if _raw_stream is not None:
        idx = t.device.index
        return C.c_void_p(_raw_stream(torch.cuda.current_device() if idx is None else idx))
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def need_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("rtfs_net_amd kernels run on the MI355X only: got a CPU tensor (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"rtfs_net_amd kernels are float32; got {t.dtype}")


def poison_byte(value):
    """The fill byte an ``RTFS_POISON_WS`` value selects: None (unset, empty, "0": off), 0xFF ("1", "nan": NaN as f32 and f64) or
    0x7F ("big": 3.4e38 as f32, 1.4e306 as f64; finite, so it survives the fmaxf of a ReLU or max-pool epilogue and blows up later)."""
    v = (value or "").strip().lower()
    if v in ("", "0"):
        return None
    if v in ("1", "nan"):
        return 0xFF
    if v == "big":
        return 0x7F
    raise ValueError(f"RTFS_POISON_WS={value!r}: expected 0, 1, nan or big")


# read at call time (tests switch it in-process with monkeypatch.setattr(_lib, "_POISON", 0xFF))
_POISON = poison_byte(os.environ.get("RTFS_POISON_WS"))
GUARD_BYTES = 64 << 10
_tls = threading.local()


def _guards():
    g = getattr(_tls, "guards", None)
    if g is None:
        g = _tls.guards = []
    return g


def _poison(t: torch.Tensor):
    if t.is_floating_point():
        t.untyped_storage().fill_(_POISON)
    return t


def empty(*size, device, dtype=torch.float32):
    """torch.empty for the outputs and saved state a C call fills.  Off, it is exactly torch.empty; under RTFS_POISON_WS a floating
    tensor comes back filled with the poison byte, so an element no kernel writes (or a kernel reads before writing) shows up."""
    t = torch.empty(*size, device=device, dtype=dtype)
    return t if _POISON is None else _poison(t)


def empty_like(t: torch.Tensor):
    """torch.empty_like with the poison fill of ``empty``."""
    e = torch.empty_like(t)
    return e if _POISON is None else _poison(e)


def workspace(nbytes: int, device):
    """Caller-owned scratch for one C call.  The kernels must never read a workspace byte they have not written in the same call;
    RTFS_POISON_WS (tests) fills every workspace with the poison byte so such a read shows up in the output, and follows it with a
    poisoned guard band of GUARD_BYTES that the next check() verifies: a write past the size the *_workspace_bytes query promised
    raises there, naming the entry point."""
    n = max(int(nbytes), 256)
    if _POISON is None:
        return torch.empty(n, dtype=torch.uint8, device=device)
    buf = torch.empty(n + GUARD_BYTES, dtype=torch.uint8, device=device)
    buf.fill_(_POISON)
    _guards().append(buf[n:])
    return buf[:n]


def _check_guards(what: str):
    """Verify (and forget) the guard bands this thread handed out since the previous check.  Skipped while the current stream is
    capturing a graph: nothing has run yet."""
    g = _guards()
    if not g:
        return
    if any(t.is_cuda for t in g) and torch.cuda.is_current_stream_capturing():
        g.clear()
        return
    pending = list(g)
    g.clear()
    if any(t.is_cuda for t in pending):
        torch.cuda.synchronize()
    bad = [t for t in pending if bool(t.ne(_POISON).any())]
    if bad:
        raise RuntimeError(f"{what} wrote past the end of {len(bad)} of its {len(pending)} workspace(s) "
                           f"(guard band of {GUARD_BYTES} bytes changed)")
