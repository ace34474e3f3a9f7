"""ctypes binding of libtalkshow_hip.so (C ABI: include/talkshow_hip.h; tuning / test aids: include/talkshow_hip_debug.h).

There is NO fallback: if the library has not been built, or no gfx950 device is present when a context is
requested, this module raises.  PyTorch is imported first on purpose — the library must share the HIP runtime
instance that owns the torch tensors whose device pointers it is handed.
"""
import ctypes as C
import os

import numpy as np
import torch  # noqa: F401  (loads libamdhip64 before ours)

_HERE = os.path.dirname(os.path.abspath(__file__))
# TS_LIB_PATH: another build of the same library (the AddressSanitizer build of `make asan`, an A/B build of tools/ab_libs.sh); it must
# export every symbol of include/*.h like the default one (load() checks)
LIB_PATH = os.environ.get("TS_LIB_PATH") or os.path.join(_HERE, "lib", "libtalkshow_hip.so")

TS_SAMPLE_GREEDY, TS_SAMPLE_UNIFORMS, TS_SAMPLE_PHILOX, TS_TEACHER_FORCED = 0, 1, 2, 3


class TsTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


_vp, _i, _i64, _u64, _fp = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.POINTER(C.c_float)


class TsSampling(C.Structure):
    """ts_sampling (include/talkshow_hip.h): the sampling record of one clip; neutral = (1.0, 1.0, 0, 0)."""
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32), ("reserved", C.c_int32)]


_sp = C.POINTER(TsSampling)


class TsRepeat(C.Structure):
    """ts_repeat (include/talkshow_hip.h, "repetition penalty"): the record of one clip; window 0 = off."""
    _fields_ = [("window", C.c_int32), ("presence", C.c_float), ("frequency", C.c_float), ("reserved", C.c_int32)]


_rp = C.POINTER(TsRepeat)


class TsAltOut(C.Structure):
    """ts_alt_out (include/talkshow_hip.h, "alternatives"): n and the four device arrays a pass fills."""
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("codes_dev", C.c_void_p), ("logprob_dev", C.c_void_p), ("entropy_dev", C.c_void_p),
                ("rank_dev", C.c_void_p)]


_ap = C.POINTER(TsAltOut)
TS_ALT_MAX = 8
TS_REPEAT_MAX_WINDOW = 64
TS_SLOT_STATE_VERSION = 1


class TsSlotInfo(C.Structure):
    """ts_slot_info (include/talkshow_hip.h, "slot state"): the host record beside one slot's state row."""
    _fields_ = [("D", C.c_int32), ("NL", C.c_int32), ("NC", C.c_int32), ("V", C.c_int32), ("version", C.c_int32), ("hist", C.c_int32),
                ("rows", C.c_int64), ("clip_index", C.c_int64), ("label", C.c_int64)]


class SkinnySeg(C.Structure):
    """ts_debug_skinny_seg (include/talkshow_hip_debug.h)."""
    _fields_ = [("base", _vp), ("gidx", _vp), ("row_stride", C.c_long), ("gidx_stride", C.c_long), ("row_shift", _i), ("len", _i),
                ("tiled_w", _i)]


class SkinnyProblem(C.Structure):
    """ts_debug_skinny_problem (include/talkshow_hip_debug.h): one chain problem, the fields of csrc/kernels.h::SkinnyParams."""
    _fields_ = [("M", _i), ("N", _i), ("nseg", _i), ("seg", SkinnySeg * 3), ("W", _vp), ("ldw", C.c_long), ("bias", _vp),
                ("add1", _vp), ("add1_stride", C.c_long), ("add1_shift", _i), ("add2", _vp), ("add2_stride", C.c_long), ("add2_shift", _i),
                ("add3", _vp), ("add3_stride", C.c_long), ("clsrow", _vp), ("cls_ld", _i), ("epi", _i), ("relu", _i), ("gateD", _i),
                ("out", _vp), ("out_stride", C.c_long), ("pre", _vp), ("pre_stride", C.c_long), ("w_tiled", _i), ("out_tiled_w", _i),
                ("pre_tiled_w", _i), ("add1_tiled_w", _i)]


class ConvSeg(C.Structure):
    """ts_debug_conv_seg (include/talkshow_hip_debug.h)."""
    _fields_ = [("d", _i), ("c0", _i), ("len", _i), ("ntap", _i)]


class ConvGroup(C.Structure):
    """ts_debug_conv_group (include/talkshow_hip_debug.h)."""
    _fields_ = [("x", _vp), ("w", _vp), ("bias", _vp), ("res", _vp), ("out", _vp), ("out_col0", _i), ("nseg", _i), ("seg", ConvSeg * 4)]


class ConvProblem(C.Structure):
    """ts_debug_conv_problem (include/talkshow_hip_debug.h): one conv_gemm_f32 launch, the fields of csrc/kernels.h::ConvParams."""
    _fields_ = [("M", _i), ("Lout", _i), ("Lin", _i), ("stride", _i), ("ldx", _i), ("ldo", _i), ("ldr", _i), ("N", _i), ("Ktot", _i),
                ("act", _i), ("ngroups", _i), ("g", ConvGroup * 4), ("res_after_act", _i), ("ldw", C.c_long), ("w_rows", _i), ("zdiv", _i),
                ("x_zs0", C.c_long), ("x_zs1", C.c_long), ("w_zs0", C.c_long), ("w_zs1", C.c_long), ("o_zs0", C.c_long),
                ("o_zs1", C.c_long), ("b_zs1", C.c_long), ("r_zs0", C.c_long), ("r_zs1", C.c_long), ("sk_ok", _i), ("lens", _vp),
                ("len_shr", _i), ("len_shl", _i), ("w_planes", _i)]


class TrunkTaps(C.Structure):
    """ts_debug_trunk_tap_table (include/talkshow_hip_debug.h): device pointers enc[network][stage], dec[network][stage], null = no tap."""
    _fields_ = [("enc", (_vp * 6) * 2), ("dec", (_vp * 6) * 2)]


PIX_TAP_STAGES = ("HV", "OV", "P", "Q1", "Q0", "V2H", "G", "XH", "T0", "Y", "LG")


class PixTaps(C.Structure):
    """ts_debug_pix_tap_table (include/talkshow_hip_debug.h): the rows to tap and one device pointer per stage of PIX_TAP_STAGES."""
    _fields_ = [("row", C.c_int32), ("row0", C.c_int32), ("rows", C.c_int32), ("slab_clips", C.c_int32),
                ("stage", _vp * len(PIX_TAP_STAGES))]


# name -> (restype, argtypes); every symbol include/*.h declares
SIGNATURES = {
    "ts_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "ts_ctx_destroy": (None, [_vp]),
    "ts_last_error": (C.c_char_p, []),
    "ts_version": (C.c_char_p, []),
    "ts_stream_create": (_i, [_vp, C.POINTER(_vp)]),
    "ts_stream_create_cus": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "ts_debug_skinny_trace": (_i, [C.POINTER(C.c_uint64), _i]),
    "ts_debug_clock_sample": (_i, [_vp, _i, _i, _vp]),
    "ts_debug_conv_bands": (_i, [_i, _i, _i, C.POINTER(_i)]),
    "ts_debug_split_tile": (_i, [_i, _i, _i, _i, C.POINTER(_i)]),
    "ts_debug_tile_weights": (_i, [_vp, _i, _i, C.c_long, _i, _i, _vp]),
    "ts_assemble_full": (_i, [_vp, _vp, _i, _vp, _i, _i, _fp, _vp, _vp]),
    "ts_assemble_full_mixed": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _fp, _vp, _vp]),
    "ts_stream_destroy": (_i, [_vp, _vp]),
    "ts_audioenc_create": (_i, [_vp, C.POINTER(TsTensor), _i, _i, _i, _i, C.POINTER(_vp)]),
    "ts_convnet_destroy": (None, [_vp]),
    "ts_audioenc_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ts_vqvae_create": (_i, [_vp, C.POINTER(TsTensor), _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "ts_vqvae_destroy": (None, [_vp]),
    "ts_vqvae_encode": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "ts_vqvae_decode": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "ts_vqvae_decode_z": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "ts_vqvae_decode_pair": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ts_vqvae_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    "ts_pixelcnn_create": (_i, [_vp, C.POINTER(TsTensor), _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "ts_pixelcnn_destroy": (None, [_vp]),
    "ts_pixelcnn_generate": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _u64, _i64, _vp, _vp, _vp, _vp, _i, _vp]),
    "ts_sampling_check": (_i, [_sp, _i, _i]),
    "ts_pixelcnn_generate_ctl": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _u64, _i64, _vp, _vp, _vp, _vp, _i, _sp, _i, _vp]),
    "ts_op_sample_ctl": (_i, [_vp, _vp, _i, _i, _i, _vp, _u64, _i64, C.c_uint32, _sp, _i, _vp, _vp, _vp]),
    # the _ctl entries plus logprob_dev ahead of the stream
    "ts_pixelcnn_generate_lp": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _u64, _i64, _vp, _vp, _vp, _vp, _i, _sp, _i, _vp, _vp]),
    "ts_op_sample_lp": (_i, [_vp, _vp, _i, _i, _i, _vp, _u64, _i64, C.c_uint32, _sp, _i, _vp, _vp, _vp, _vp]),
    "ts_logprob_sums": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ts_given_rows_check": (_i, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i]),
    # given poses: the mixed VQ encode
    "ts_vqvae_encode_pair_masked": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "ts_body_vq_infer_mixed": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ts_given_pose_rows_check": (_i, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i]),
    "ts_op_vq_argmin_pair_masked": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ts_debug_vq_argmin_pair_masked": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "ts_op_sample_given": (_i, [_vp, _vp, _i, _i, _i, _vp, _u64, _i64, C.c_uint32, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp]),
    # kept positions: the one-launch form with the device-side decision
    "ts_op_sample_keep": (_i, [_vp, _vp, _i, _i, _i, _vp, _u64, _i64, C.c_uint32, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _vp]),
    # speaker style: the host rule; the kernel alone
    "ts_style_check": (_i, [C.POINTER(C.c_float), C.c_long, _i]),
    "ts_op_style_rows": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    # code bias: the host rules; one launch
    "ts_code_bias_check": (_i, [C.POINTER(C.c_float), _i, _i]),
    "ts_code_bias_index_check": (_i, [C.POINTER(C.c_int32), _i, _i]),
    "ts_op_sample_bias": (_i, [_vp, _vp, _i, _i, _i, _vp, _u64, _i64, C.c_uint32, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp,
                               _i, C.POINTER(C.c_int32), _i, _vp]),
    # repetition penalty: the host rule; one launch
    "ts_repeat_check": (_i, [_rp, _i, _i]),
    "ts_op_sample_repeat": (_i, [_vp, _vp, _i, _i, _i, _vp, _u64, _i64, C.c_uint32, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp,
                                 _i, C.POINTER(C.c_int32), _i, _rp, _i, _vp, _vp, _vp]),
    # guidance: the host rule; one launch (ts_op_sample_repeat's arguments, then guide_host and guide_scale_host ahead of the stream)
    "ts_guide_check": (_i, [C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int32), _i]),
    "ts_op_sample_guide": (_i, [_vp, _vp, _i, _i, _i, _vp, _u64, _i64, C.c_uint32, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp,
                                _i, C.POINTER(C.c_int32), _i, _rp, _i, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), _vp]),
    # alternatives: the host rule; one launch (ts_op_sample_repeat's arguments, then the record ahead of the stream)
    "ts_alt_check": (_i, [_ap, _i]),
    "ts_op_sample_alt": (_i, [_vp, _vp, _i, _i, _i, _vp, _u64, _i64, C.c_uint32, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp,
                              _i, C.POINTER(C.c_int32), _i, _rp, _i, _vp, _vp, _ap, _vp]),
    "ts_pixelcnn_v_create": (_i, [_vp, C.POINTER(TsTensor), _i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "ts_pixelcnn_v_destroy": (None, [_vp]),
    "ts_pixelcnn_v_generate": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _u64, _i64, _vp, _vp, _vp, _vp, _i, _vp]),
    "ts_pixelcnn_stream_open": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "ts_pixelcnn_stream_step": (_i, [_vp, _vp, _i, _i, _vp, _u64, _i64, _vp, _vp]),
    # the step plus ctl / n_ctl, logprob, given / given_rows, style, bias / n_bias / bias_index, rep / n_rep ahead of the stream
    "ts_pixelcnn_stream_step_ctl": (_i, [_vp, _vp, _i, _i, _vp, _u64, _i64, _vp, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _i,
                                         C.POINTER(C.c_int32), _rp, _i, _vp]),
    # the step plus the alternatives record ahead of the stream
    "ts_pixelcnn_stream_step_alt": (_i, [_vp, _vp, _i, _i, _vp, _u64, _i64, _vp, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _i,
                                         C.POINTER(C.c_int32), _rp, _i, _ap, _vp]),
    "ts_pixelcnn_stream_captures": (_i64, [_vp]),
    "ts_debug_rep_table": (_i, [_rp, _i, _i, _i, C.POINTER(C.c_int32)]),
    "ts_pixelcnn_stream_rows": (_i64, [_vp]),
    "ts_pixelcnn_stream_close": (None, [_vp]),
    # slot restart: slots (n,) host, n, labels (n,) host or NULL, style (n,NC) device or NULL, clip indices (n,) host, stream
    "ts_pixelcnn_stream_restart": (_i, [_vp, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int64), _vp, C.POINTER(C.c_int64), _vp]),
    "ts_pixelcnn_stream_slot_rows": (_i64, [_vp, _i]),
    # slot state: slots (n,) host, n, state (n, words) device, info (n,) host, stream / ... states, n_states, index (n,) host or NULL, info
    # (n_states,) host, clip indices (n,) host or NULL, stream
    "ts_pixelcnn_slot_state_words": (_i64, [_vp]),
    "ts_pixelcnn_stream_save": (_i, [_vp, C.POINTER(C.c_int32), _i, _vp, C.POINTER(TsSlotInfo), _vp]),
    "ts_pixelcnn_stream_load": (_i, [_vp, C.POINTER(C.c_int32), _i, _vp, _i, C.POINTER(C.c_int32), C.POINTER(TsSlotInfo), C.POINTER(C.c_int64), _vp]),
    "ts_pixelcnn_stream_graph_stats": (_i, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(C.c_double)]),
    # session pairs: primary / shadow / scale (n,) host, n; the (S,) table out; step_ctl plus guide_scale (S,) host ahead of the stream;
    # the host rule: S, rows, guide (S,), clip rows (S,), fresh (S,), primary (n,), shadow (n,) or NULL, scale (n,) or NULL, n
    "ts_pixelcnn_stream_pair": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), _i]),
    "ts_pixelcnn_stream_pairs": (_i, [_vp, C.POINTER(C.c_int32)]),
    "ts_pixelcnn_stream_step_guided": (_i, [_vp, _vp, _i, _i, _vp, _u64, _i64, _vp, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _i,
                                            C.POINTER(C.c_int32), _rp, _i, C.POINTER(C.c_float), _vp]),
    "ts_pixelcnn_stream_pair_check": (_i, [_i, _i64, C.POINTER(C.c_int32), C.POINTER(_i64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_float), _i]),
    # seamless sessions: the step's arguments around (mfcc, t) / the two outputs, then the pieces of ts_pixelcnn_stream_step_ctl
    "ts_body_stream_open": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(_vp)]),
    "ts_body_stream_plan": (_i, [_vp, _i, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "ts_body_stream_push": (_i, [_vp, _vp, _i, _i, _vp, _u64, _i64, _vp, _vp, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _i,
                                 C.POINTER(C.c_int32), _rp, _i, _vp]),
    "ts_body_stream_flush": (_i, [_vp, _i, _vp, _u64, _i64, _vp, _vp, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _i,
                                  C.POINTER(C.c_int32), _rp, _i, _vp]),
    # guided sessions: ids (S,) device, B, n_shadow, shadow_of / enc_of (n_shadow,) host, style (n_shadow,NC) device or NULL, scales
    # (n_shadow,) host, max frames, stream, out; push / flush plus guide_scale (S,) host ahead of the stream
    "ts_body_stream_open_guided": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, C.POINTER(C.c_float),
                                        _i, _vp, C.POINTER(_vp)]),
    "ts_body_stream_push_guided": (_i, [_vp, _vp, _i, _i, _vp, _u64, _i64, _vp, _vp, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _i,
                                        C.POINTER(C.c_int32), _rp, _i, C.POINTER(C.c_float), _vp]),
    "ts_body_stream_flush_guided": (_i, [_vp, _i, _vp, _u64, _i64, _vp, _vp, _sp, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _i,
                                         C.POINTER(C.c_int32), _rp, _i, C.POINTER(C.c_float), _vp]),
    "ts_body_stream_frames_in": (_i64, [_vp]),
    "ts_body_stream_code_rows": (_i64, [_vp]),
    "ts_body_stream_pose_frames": (_i64, [_vp]),
    "ts_body_stream_state_bytes": (_i64, [_vp]),
    "ts_body_stream_captures": (_i64, [_vp]),
    "ts_body_stream_close": (None, [_vp]),
    "ts_body_stream_lag_rows": (_i, [_vp]),
    "ts_debug_body_stream_plan": (_i, [C.POINTER(_i64), _i, _i, _i, C.POINTER(_i64)]),
    # the staging and glue kernels alone (tests/test_gpu_glue_ops.py)
    "ts_debug_stream_stage_mfcc": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "ts_debug_stream_emit": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "ts_debug_stream_keep_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "ts_debug_stream_spread_rows": (_i, [_vp, _vp, C.POINTER(C.c_int32), _i, _i, _i, _i, _i, _i, _vp]),
    "ts_debug_gather_rows": (_i, [_vp, _i, _i, _vp, C.c_long, _i, _i, _vp, _i, _i, _vp, _i, _vp]),
    "ts_debug_pad_rows": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ts_debug_mask_rows": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ts_debug_iota_i64": (_i, [_vp, _i, _i64, _vp]),
    "ts_debug_i64_to_i32": (_i, [_vp, _vp, C.c_long, _vp]),
    "ts_debug_set_words3": (_i, [_vp, _u64, _u64, _u64, _vp]),
    "ts_debug_row_sqnorm": (_i, [_vp, _i, _i, _vp, _vp]),
    "ts_debug_slot_save": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i] + [_vp] * 11),
    "ts_debug_slot_load": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i] + [_vp] * 9),
    "ts_face_create": (_i, [_vp, C.POINTER(TsTensor), _i, _i, _i, C.POINTER(_vp)]),
    "ts_face_destroy": (None, [_vp]),
    "ts_face_generate": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ts_face_generate_mixed": (_i, [_vp, _vp, C.POINTER(C.c_int32), _vp, C.POINTER(C.c_int32), _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ts_face_mixed_rows": (_i, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _i, _i, C.POINTER(_i64)]),
    "ts_face_set_arith": (_i, [_vp, _i]),
    "ts_mfcc_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "ts_mfcc_destroy": (None, [_vp]),
    "ts_mfcc_num_frames": (_i, [_vp, C.c_long]),
    "ts_mfcc_forward": (_i, [_vp, _vp, _i, C.c_long, _vp, _vp]),
    "ts_mfcc_resampled_len": (C.c_long, [_vp, C.c_long]),
    "ts_mfcc_resample": (_i, [_vp, _vp, _i, C.c_long, _vp, _vp]),
    "ts_resample_kaiser_len": (C.c_long, [C.c_long, _i, _i]),
    "ts_resample_kaiser": (_i, [_vp, _vp, _i, C.c_long, _i, _i, _vp, _vp]),
    "ts_mfcc_forward_mixed": (_i, [_vp, _vp, C.POINTER(C.c_int32), _vp, _i, C.c_long, _vp, _vp]),
    "ts_mfcc_resample_mixed": (_i, [_vp, _vp, C.POINTER(C.c_int32), _vp, _i, C.c_long, _vp, _vp]),
    "ts_resample_kaiser_mixed": (_i, [_vp, _vp, C.POINTER(C.c_int32), _vp, _i, C.c_long, _i, _i, _vp, _vp]),
    "ts_mfcc_peak_db_mixed": (_i, [_vp, _vp, C.POINTER(C.c_int32), _vp, _i, C.c_long, _vp, _vp]),
    # wav sessions (talkshow_hip.h, "wav sessions")
    "ts_mfcc_stream_open": (_i, [_vp, _i, C.c_long, _i, _vp, C.POINTER(_vp)]),
    "ts_mfcc_stream_push": (_i, [_vp, _vp, C.c_long, _vp, C.POINTER(_i), _vp]),
    "ts_mfcc_stream_flush": (_i, [_vp, _vp, C.POINTER(_i), _vp]),
    "ts_mfcc_stream_samples_in": (C.c_long, [_vp]),
    "ts_mfcc_stream_frames_out": (C.c_long, [_vp]),
    "ts_mfcc_stream_state_bytes": (C.c_long, [_vp]),
    "ts_mfcc_stream_max_frames": (C.c_long, [_vp]),
    "ts_mfcc_stream_close": (None, [_vp]),
    "ts_mfcc_stream_plan": (_i, [_i, _i, _i, C.c_long, C.c_long, _i, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "ts_mfcc_constants": (None, [_vp, C.POINTER(C.c_int32)]),
    "ts_debug_mfcc_stream_tap": (_i, [_vp, _vp, C.c_long, _vp, C.c_long]),
    "ts_debug_mfcc_stream_tails": (None, [_vp, C.POINTER(C.c_long)]),
    "ts_debug_mfcc_stream_db": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ts_debug_mfcc_stft": (_i, [_vp, _vp, _i, C.c_long, _vp, _vp]),
    "ts_debug_mfcc_stft_lens": (_i, [_vp, _vp, C.POINTER(C.c_int32), _vp, _i, C.c_long, _vp, _vp]),
    "ts_debug_mfcc_frames": (_i, [_vp, _vp, _i, C.c_long, _vp, _vp]),
    "ts_debug_mfcc_mel": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ts_debug_mfcc_db": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "ts_debug_mfcc_dct": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ts_pixelcnn_graph_stats": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_i64), C.POINTER(C.c_double)]),
    "ts_body_pixel_infer": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _u64, _i64, _vp, _vp, _vp]),
    "ts_body_pixel_infer_mixed": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp, _vp]),
    "ts_audioenc_forward_masked": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ts_pixelcnn_generate_mixed": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp]),
    "ts_vqvae_decode_pair_masked": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ts_debug_mixed_plan": (_i, [C.POINTER(C.c_int32), _i, _i, C.POINTER(C.c_int32)]),
    "ts_body_vq_infer": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ts_op_conv1d": (_i, [_vp, _vp, _i, _i, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "ts_op_conv1d_timed": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, C.POINTER(C.c_float), _vp]),
    "ts_op_conv_taps48_timed": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, C.POINTER(C.c_float), _vp]),
    "ts_op_conv1d_strided_timed": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, C.POINTER(C.c_float), _vp]),
    "ts_debug_pixelcnn_graphs": (_i, [_vp, _vp]),
    "ts_debug_code_tables_plan": (_i, [_i, _i, _i, _i, _i, _i, C.c_char_p, C.POINTER(_i64)]),
    "ts_debug_pixelcnn_tables": (_i, [_vp, _i]),
    "ts_debug_pixelcnn_work": (_i64, [_vp, _vp, _i, _vp, _i64, _i]),
    "ts_debug_code_table_stage": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ts_debug_conv_run": (_i, [_vp, C.POINTER(ConvProblem), _i, C.c_char_p, _i, C.POINTER(_i), _vp]),
    "ts_debug_conv_sk_plan": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int)]),
    "ts_debug_conv_sk_run": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int)]),
    "ts_debug_conv_sk_supported": (_i, []),
    "ts_pixelcnn_graph_captures": (C.c_long, [_vp, _vp]),
    "ts_pixelcnn_prepare": (_i, [_vp, _i, _i, _i, _vp]),
    "ts_debug_wino_lowering": (_i, [_i, _i, _i, _i, C.c_char_p, _i, _i, C.POINTER(_i)]),
    "ts_debug_wino_weights": (_i, [_vp, _i, _i, _vp]),
    "ts_debug_wino_transform": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, C.POINTER(_vp), _vp]),
    "ts_debug_wino_gemm": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "ts_debug_wino_codes": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ts_debug_vqvae_dec_tables": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "ts_debug_trunk_taps": (_i, [C.POINTER(TrunkTaps)]),
    "ts_debug_pixelcnn_taps": (_i, [C.POINTER(PixTaps)]),
    "ts_debug_conv_plan": (_i, [_i, _i, _i, _i, _i, C.POINTER(_i), _i, _i, C.c_char_p, C.POINTER(_i)]),
    "ts_debug_skinny_plan": (_i, [C.POINTER(_i), _i, C.c_char_p, C.POINTER(_i)]),
    "ts_debug_skinny_run": (_i, [_vp, C.POINTER(SkinnyProblem), _i, C.c_char_p, C.POINTER(_i), _vp]),
    "ts_debug_gate_act": (_i, [_vp, _vp, _vp, C.c_long, _vp]),
    "ts_debug_gelu": (_i, [_vp, _vp, C.c_long, _vp]),
    "ts_debug_attention": (_i, [_vp, _i, _i, _i, _i, C.c_float, _vp, _vp]),
    "ts_debug_layernorm_rows": (_i, [_vp, _i, C.c_long, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "ts_debug_lerp_ln": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ts_debug_w2v_conv0": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "ts_debug_fill_id": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "ts_debug_attention_mixed": (_i, [_vp, C.POINTER(C.c_int32), _vp, _i, _i, _i, _i, C.c_float, _vp, _vp]),
    "ts_debug_layernorm_rows_lens": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "ts_debug_lerp_ln_lens": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ts_debug_w2v_conv0_lens": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "ts_debug_fill_id_lens": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ts_debug_face_mixed_grid": (_i, [C.POINTER(C.c_int32), _i, _i, C.POINTER(C.c_int32), _i]),
    "ts_debug_face_packed_layout": (_i, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "ts_debug_face_generate_mixed": (_i, [_vp, _vp, C.POINTER(C.c_int32), _vp, C.POINTER(C.c_int32), _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i]),
    "ts_debug_attention_packed": (_i, [_vp, C.POINTER(C.c_int32), _vp, _i, _i, _i, C.c_float, _vp, _vp]),
    "ts_debug_pack_rows": (_i, [_vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp]),
    "ts_debug_unpack_rows": (_i, [_vp, C.POINTER(C.c_int32), _vp, _i, _i, _i, _vp, _vp]),
    "ts_debug_w2v_conv0_packed": (_i, [_vp, _i, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "ts_debug_lerp_ln_packed": (_i, [_vp, _i, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp, _vp]),
    "ts_op_vq_argmin": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "ts_op_linear": (_i, [_vp, _vp, _i, _i, _fp, _fp, _i, _i, _vp, _vp]),
    "ts_op_sample": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ts_op_sample_philox": (_i, [_vp, _vp, _i, _i, _u64, _i64, C.c_uint32, _vp, _vp]),
    "ts_debug_skinny_chain": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(C.c_float)]),
    "ts_smplx_create": (_i, [_vp, _i, _i, _i, _i, _fp, _fp, _fp, _fp, C.POINTER(C.c_int32), _fp, _fp, C.POINTER(C.c_int32), _i,
                             C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _fp, _i, C.POINTER(_vp)]),
    "ts_smplx_destroy": (None, [_vp]),
    "ts_smplx_num_joints": (_i, [_vp]),
    "ts_smplx_forward": (_i, [_vp, _vp, _i, _vp, _i, _i, _i64, _vp, _vp, _vp]),
    "ts_debug_smplx_dims": (_i, [_vp, C.POINTER(C.c_int32)]),
    "ts_debug_smplx_need": (_i, [_vp, C.POINTER(C.c_int32)]),
    "ts_debug_smplx_pose_prepare": (_i, [_vp, _vp, _i, _vp, _i, _i, _i64, _vp, _vp, _vp]),
    "ts_debug_smplx_blend": (_i, [_vp, _i, _vp, _i64, _vp, _vp]),
    "ts_debug_smplx_rigid_chain": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "ts_debug_smplx_skin": (_i, [_vp, _i, _vp, _vp, _i64, _vp, _vp]),
    "ts_debug_smplx_joints_tail": (_i, [_vp, _vp, _i64, _vp, _vp]),
    "ts_eval_feat_stats": (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    "ts_eval_l1_total": (_i, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "ts_eval_body_loss": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ts_eval_diversity": (_i, [_vp, _vp, _i, _i64, _vp, _vp]),
    "ts_prof_enable": (_i, [_vp, _i]),
    "ts_prof_read": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), _i]),
    "ts_prof_read_n": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), _i]),
}

# The suffixed mixed entries: each sibling is its parent plus one piece of arguments ahead of the stream
_i32p = C.POINTER(C.c_int32)
MIXED_CORE = {
    "ts_body_pixel_infer_mixed": [_vp, _vp, _vp, _vp, _vp, _vp, _i32p, _vp, _i, _i, _i, _vp, _u64, _vp, _vp, _vp],
    "ts_pixelcnn_generate_mixed": [_vp, _vp, _vp, _i32p, _vp, _i, _i, _i, _vp, _u64, _vp, _vp],
}
MIXED_PIECES = {
    "ctl": [_sp, _i],                 # ctl_host, n_ctl
    "lp": [_vp],                      # logprob_dev
    "given": [_vp, _i32p, _vp],       # given_dev, given_rows_host, given_rows_dev
    "poses": [_vp, _i, _i32p, _vp],   # given_poses_dev, P_max, pose_lens_host, pose_lens_dev
    "keep": [_vp],                    # keep_dev
    "style": [_vp, _i],               # style_dev, style_rows
    "bias": [_vp, _i, _i32p],         # bias_dev, n_bias, bias_index_host
    "repeat": [_rp, _i],              # rep_host, n_rep
    "guide": [_i32p, _fp],            # guide_host, guide_scale_host
    "alt": [_ap],                     # alt (the ts_alt_out record)
}


def _declare_ladder(stem, below, suffixes):
    """SIGNATURES[stem + "_" + suffix] for every suffix in turn: the pieces `below` it, its own (named by the suffix's last word) and
    those of the suffixes ahead of it, between the stem's core arguments and the stream."""
    args = MIXED_CORE[stem] + [a for piece in below for a in MIXED_PIECES[piece]]
    for suffix in suffixes:
        args = args + MIXED_PIECES[suffix.rsplit("_", 1)[-1]]
        SIGNATURES[f"{stem}_{suffix}"] = (_i, args + [_vp])


_declare_ladder("ts_body_pixel_infer_mixed", (), ("ctl", "lp", "given", "keep", "style", "bias", "repeat"))
_declare_ladder("ts_pixelcnn_generate_mixed", (), ("ctl", "lp", "given", "keep", "style", "bias", "repeat"))
_declare_ladder("ts_body_pixel_infer_mixed", ("ctl", "lp"), ("poses", "poses_keep", "poses_style", "poses_bias", "poses_repeat"))
# alternatives: the rung above the most general unguided entry of each family, under names of their own like the guided entries, named only
# by a pass that brings the record
ALT_ENTRY = {
    "ts_body_pixel_infer_mixed_repeat": "ts_body_pixel_infer_alt",
    "ts_body_pixel_infer_mixed_poses_repeat": "ts_body_pixel_infer_alt_poses",
    "ts_pixelcnn_generate_mixed_repeat": "ts_pixelcnn_generate_alt",
}
# guidance: the most general entry of each family plus the guide piece ahead of the stream, under names of their own
GUIDED_ENTRY = {
    "ts_body_pixel_infer_mixed_repeat": "ts_body_pixel_infer_guided",
    "ts_body_pixel_infer_mixed_poses_repeat": "ts_body_pixel_infer_guided_poses",
    "ts_pixelcnn_generate_mixed_repeat": "ts_pixelcnn_generate_guided",
}
for _plain, _guided in GUIDED_ENTRY.items():
    SIGNATURES[_guided] = (_i, SIGNATURES[_plain][1][:-1] + MIXED_PIECES["guide"] + [_vp])
for _plain, _alt in ALT_ENTRY.items():
    SIGNATURES[_alt] = (_i, SIGNATURES[_plain][1][:-1] + MIXED_PIECES["alt"] + [_vp])

_lib = None


def load():
    """dlopen the library and declare every prototype.  Raises if it is missing (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension is not built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise RuntimeError("libtalkshow_hip: " + load().ts_last_error().decode())


def check_value(rc):
    """`check` for a host-only rule on the caller's values: ValueError with the library's message."""
    if rc != 0:
        raise ValueError("libtalkshow_hip: " + load().ts_last_error().decode())


def fptr(a):
    """host float32 numpy array -> POINTER(c_float) (the array must outlive the call)."""
    return a.ctypes.data_as(_fp) if a is not None else None


def dptr(t):
    """torch CUDA tensor -> raw device pointer (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors handed to the C ABI must be contiguous HIP tensors"
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def face_generate_mixed(handle, wav, ns, ns_dev, frames, frames_dev, B, N_max, T_max, id_dev, out, hidden, layout=None):
    """`ts_face_generate_mixed` on the current stream; ns / frames = int32 numpy tables, the rest device tensors.  layout None = the
    library's plan (padded unless TS_FACE_PACK=1); 0 / 1 = padded / packed named through the debug entry (tests, A/B in one process)."""
    i32p = C.POINTER(C.c_int32)
    args = [handle, dptr(wav), ns.ctypes.data_as(i32p), dptr(ns_dev), frames.ctypes.data_as(i32p), dptr(frames_dev), int(B), int(N_max),
            int(T_max), dptr(id_dev), dptr(out), dptr(hidden), stream_ptr()]
    if layout is None:
        check(load().ts_face_generate_mixed(*args))
    else:
        if layout not in (0, 1):
            raise ValueError("layout is None (the library's plan), 0 (padded) or 1 (packed)")
        check(load().ts_debug_face_generate_mixed(*args, int(layout)))


def _mixed_tail(middle, ctl=None, n_ctl=0, logprob=None, keep=None, style=None, style_rows=0, bias=None, n_bias=0, bias_index=None,
                rep=None, n_rep=0, guide=None, guide_scale=None, alt=None, stream=None):
    """What follows the fixed arguments of a most general mixed entry (`..._repeat`), `middle` being its given or poses piece: every
    keyword is an already-converted value (pointer, int, ctypes array), an absent one travels as None / 0.  guide / guide_scale (the
    guided entries' piece, `GUIDED_ENTRY`) sit ahead of the stream only when a guide table came: without one the tail is the `_repeat`
    entries'."""
    tail = (ctl, int(n_ctl) if ctl is not None else 0, logprob, *middle, keep, style, int(style_rows) if style is not None else 0,
            bias, int(n_bias) if bias is not None else 0, bias_index if bias is not None else None,
            rep, int(n_rep) if rep is not None else 0)
    if guide is not None:
        if guide_scale is None:
            raise ValueError("_mixed_tail: a guide table needs its scales")
        tail += (guide, guide_scale)
    if alt is not None:      # the `_alt` entries' piece (`ALT_ENTRY`), likewise only when the record came
        if guide is not None:
            raise NotImplementedError("alternatives are not offered on a guided pass")
        tail += (alt,)
    return (*tail, stream)


def body_mixed_args(fixed, given=None, given_rows=None, poses=None, **pieces):
    """(entry name, argument tuple) of a mixed body pass: `fixed` the 16 arguments of `ts_body_pixel_infer_mixed` ahead of its stream,
    given / given_rows the device block and its host table, poses (given_poses_dev, P_max, pose_lens_host, pose_lens_dev), the rest as
    `_mixed_tail` takes it.  A pass that brings poses and no given codes is `ts_body_pixel_infer_mixed_poses_repeat`, every other one
    `ts_body_pixel_infer_mixed_repeat`: NULL is "the entry without that keyword, launch for launch" (talkshow_hip.h)."""
    if poses is not None and given is not None:
        raise ValueError("body_mixed_args: a pass brings given codes or given poses (stage the poses' codes into the given block)")
    name = "ts_body_pixel_infer_mixed_poses_repeat" if poses is not None else "ts_body_pixel_infer_mixed_repeat"
    if pieces.get("guide") is not None:      # the guided entries only for a pass that brings the table
        name = GUIDED_ENTRY[name]
    elif pieces.get("alt") is not None:        # and the alternatives entries only for a pass that brings the record
        name = ALT_ENTRY[name]
    if poses is not None:
        return name, (*fixed, *_mixed_tail(tuple(poses), **pieces))
    return name, (*fixed, *_mixed_tail((given, given_rows if given is not None else None, None), **pieces))


def body_mixed_call(fixed, **pieces):
    """`body_mixed_args` on the current stream: load, call, check."""
    name, args = body_mixed_args(fixed, stream=stream_ptr(), **pieces)
    check(getattr(load(), name)(*args))


def pixelcnn_mixed_args(fixed, given=None, given_rows=None, **pieces):
    """`body_mixed_args` for the PixelCNN alone (`fixed`: its 12 arguments ahead of the stream): always `ts_pixelcnn_generate_mixed_repeat`."""
    name = "ts_pixelcnn_generate_mixed_repeat"
    if pieces.get("guide") is not None:
        name = GUIDED_ENTRY[name]
    elif pieces.get("alt") is not None:
        name = ALT_ENTRY[name]
    return name, (*fixed, *_mixed_tail((given, given_rows if given is not None else None, None), **pieces))


def pixelcnn_mixed_call(fixed, **pieces):
    name, args = pixelcnn_mixed_args(fixed, stream=stream_ptr(), **pieces)
    check(getattr(load(), name)(*args))


NEUTRAL_SAMPLING = (1.0, 1.0, 0)


def sampling_record(rec):
    """One sampling record as (temperature, top_p, top_k) floats / int: None (neutral), a dict with any of the keys `temperature`, `top_p`,
    `top_k`, or a TUPLE (temperature, top_p, top_k).  A list is never one record: lists hold one record per clip (`sampling_records`).
    Pure host code."""
    if rec is None:
        return NEUTRAL_SAMPLING
    if isinstance(rec, dict):
        unknown = set(rec) - {"temperature", "top_p", "top_k"}
        if unknown:
            raise ValueError(f"sampling record: unknown keys {sorted(unknown)} (temperature, top_p, top_k)")
        t, p, k = rec.get("temperature"), rec.get("top_p"), rec.get("top_k")
        return (1.0 if t is None else float(t), 1.0 if p is None else float(p), 0 if k is None else int(k))
    if isinstance(rec, tuple) and len(rec) == 3:
        return (float(rec[0]), float(rec[1]), int(rec[2]))
    raise ValueError(f"a sampling record is None, a dict or a tuple (temperature, top_p, top_k), got {rec!r}")


def sampling_records(sampling, n):
    """`sampling` as a list of n records: None / a dict / a 3-tuple is ONE record for all clips, a LIST of n entries (each None, a dict or a
    3-tuple) is one per clip.  A single record written as a list, `[0.9, 0.95, 64]`, is refused with a message that says so."""
    if sampling is None or isinstance(sampling, (dict, tuple)):
        return [sampling_record(sampling)] * n
    if not isinstance(sampling, list):
        raise ValueError(f"sampling must be None, a dict, a tuple (temperature, top_p, top_k) or a list of one record per clip, got {sampling!r}")
    recs = sampling
    if recs and all(isinstance(r, (int, float)) for r in recs):
        raise ValueError(f"sampling={recs!r}: a list holds one record per clip; write one record for all clips as a tuple (temperature, top_p, top_k)")
    if len(recs) != n:
        raise ValueError(f"sampling must hold one record or one per clip ({n}), got {len(recs)}")
    return [sampling_record(r) for r in recs]


def sampling_table(sampling, n, V=2048, mode=None):
    """A validated `ts_sampling` table of n records (ts_sampling_check: a bad record raises ValueError naming the clip) -> (array, n).  With
    `mode`, a table for a mode that draws nothing (greedy, teacher forced) is refused here as the C entries refuse it."""
    if mode is not None and mode not in (TS_SAMPLE_UNIFORMS, TS_SAMPLE_PHILOX):
        raise ValueError("sampling controls need TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX (per-clip greedy is top_k = 1)")
    recs = sampling_records(sampling, n)
    arr = (TsSampling * n)()
    for b, (t, p, k) in enumerate(recs):
        if not -2 ** 31 <= k < 2 ** 31:
            raise ValueError(f"sampling record of clip {b}: top_k out of range")
        arr[b].temperature, arr[b].top_p, arr[b].top_k, arr[b].reserved = t, p, k, 0
    lib = load()
    if lib.ts_sampling_check(arr, n, int(V)) != 0:
        raise ValueError("libtalkshow_hip: " + lib.ts_last_error().decode())
    return arr, n


def logprob_request(logprobs, shape, device=None):
    """The `logprobs=` keyword of the decode entries: False / None -> None (no output, the entries without the suffix); True -> "new" (the
    entry allocates a float32 tensor of `shape`, the codes' shape); a tensor -> that tensor, which must be float32, contiguous, of `shape`
    and, where `device` is given, on it.  Anything else, or a wrong tensor, raises ValueError: pure host code, ahead of any launch."""
    if logprobs is None or logprobs is False:
        return None
    if logprobs is True:
        return "new"
    dtype, tshape = getattr(logprobs, "dtype", None), getattr(logprobs, "shape", None)
    if dtype is None or tshape is None or not hasattr(logprobs, "is_contiguous"):
        raise ValueError(f"logprobs must be True, False or a float32 output tensor of shape {tuple(shape)}, got {logprobs!r}")
    if "float32" not in str(dtype):
        raise ValueError(f"logprobs output must be float32, got {dtype}")
    if tuple(tshape) != tuple(shape):
        raise ValueError(f"logprobs output must have the codes' shape {tuple(shape)}, got {tuple(tshape)}")
    if not logprobs.is_contiguous():
        raise ValueError("logprobs output must be contiguous")
    if device is not None and str(logprobs.device).split(":")[0] != str(device).split(":")[0]:
        raise ValueError(f"logprobs output must live on {device}, got {logprobs.device}")
    return logprobs


class AltRequest:
    """The `alternatives=n` keyword of one call: the four device tensors over `shape` (the codes' positions, (..., 2)) and the ts_alt_out
    record that names them.  `result()` is what the call appends to its return value."""

    def __init__(self, n, shape, device):
        self.n = int(n)
        shape = tuple(int(x) for x in shape)
        self.codes = torch.empty(shape + (self.n,), dtype=torch.int32, device=device)
        self.logprobs = torch.empty(shape + (self.n,), dtype=torch.float32, device=device)
        self.entropy = torch.empty(shape, dtype=torch.float32, device=device)
        self.rank = torch.empty(shape, dtype=torch.int32, device=device)
        self.record = TsAltOut(self.n, 0, self.codes.data_ptr() if self.n else None, self.logprobs.data_ptr() if self.n else None,
                               self.entropy.data_ptr(), self.rank.data_ptr())

    def ptr(self):
        return C.pointer(self.record)

    def result(self, index=None):
        """sampling.Alternatives of the whole block, or of rows `index` (an int64 device tensor) of its first axis."""
        from . import sampling
        pick = (lambda t: t) if index is None else (lambda t: t.index_select(0, index))
        return sampling.Alternatives(pick(self.codes).long(), pick(self.logprobs), pick(self.entropy), pick(self.rank).long())


def alt_request(alternatives, mode, who, guide=False):
    """The `alternatives=` keyword, checked before any device work: None -> None (the entries without the record); otherwise n in [0, 8]
    (ValueError), a drawing mode (ValueError: greedy is sampling=(1, 1, 1) under Philox) and no guidance (NotImplementedError)."""
    if alternatives is None:
        return None
    from . import sampling
    n = sampling.alt_count(alternatives)
    if mode not in (TS_SAMPLE_UNIFORMS, TS_SAMPLE_PHILOX):
        raise ValueError(f"{who}: alternatives need a drawing mode (TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX); a greedy decode with "
                         "alternatives is sampling=(1, 1, 1) under TS_SAMPLE_PHILOX")
    if guide:
        raise NotImplementedError(f"{who}: alternatives are not offered on a guided pass or a session with pairs")
    return n


def given_block(given, rows, V, order=None, who="given", keep=None):
    """The `given=` keyword of the decode entries -> (block (B, max rows, 2) int64, table (B,) int32), both numpy, both in SLOT order: what
    `ts_body_pixel_infer_mixed_given` / `ts_pixelcnn_generate_mixed_given` take as given_dev (after an upload) and given_rows_host.
    given: a list in SUBMISSION order with None (nothing given: G = 0) or a (G_b, 2) integer array per clip, or one (B, G, 2) integer block;
    rows: every clip's own code rows H_b in submission order; V: the vocabulary; order: sorted slot k holds submitted clip order[k] (None:
    the submitted order).  Rows of the block at or beyond a clip's G_b are 0 (the pass never reads them).  ValueError naming the SUBMITTED
    clip for a bad shape, a non-integer array, G_b > H_b, or a code outside [0, V).  Pure host code; a device tensor is read back.
    keep: the pass's mask of kept positions (`given_keep_block`: (B, max rows, 2) uint8, slot order) or None.  With a mask the vocabulary
    rule applies to KEPT positions only — an unkept code is never read by the pass and may hold anything — and unkept entries of the block
    are 0."""
    B = len(rows)
    if hasattr(given, "detach"):
        given = given.detach().cpu().numpy()
    if isinstance(given, np.ndarray):
        if given.ndim != 3 or given.shape[0] != B or given.shape[2] != 2:
            raise ValueError(f"{who}: one block for all clips must have shape (B={B}, G, 2), got {tuple(given.shape)}")
        given = list(given)
    if not isinstance(given, (list, tuple)) or len(given) != B:
        raise ValueError(f"{who}: one entry per clip ({B}) — None or a (G, 2) integer array — or one (B, G, 2) block, got "
                         f"{type(given).__name__}" + (f" of {len(given)}" if isinstance(given, (list, tuple)) else ""))
    order = list(range(B)) if order is None else [int(i) for i in order]
    if sorted(order) != list(range(B)):
        raise ValueError(f"{who}: order must be a permutation of the {B} clips")
    block = np.zeros((B, max(int(h) for h in rows), 2), np.int64)
    table = np.zeros(B, np.int32)
    for k, i in enumerate(order):
        g = given[i]
        if g is None:
            continue
        if hasattr(g, "detach"):
            g = g.detach().cpu().numpy()
        g = np.asarray(g)
        if g.ndim != 2 or g.shape[1] != 2:
            raise ValueError(f"{who}: given rows of clip {i} must have shape (G, 2), got {tuple(g.shape)}")
        if g.dtype.kind not in "iu":
            raise ValueError(f"{who}: given rows of clip {i} must be integers, got {g.dtype}")
        if g.shape[0] > int(rows[i]):
            raise ValueError(f"{who}: clip {i} brings {g.shape[0]} given rows but has {int(rows[i])} code rows of its own")
        if keep is not None:       # what the pass reads of this clip: its kept positions
            g = np.where(np.asarray(keep[k, :g.shape[0]]) != 0, g, np.zeros_like(g))
        if g.size and (int(g.min()) < 0 or int(g.max()) >= int(V)):
            bad = g[(g < 0) | (g >= int(V))]
            raise ValueError(f"{who}: given rows of clip {i} hold the code {int(bad.flat[0])}, outside [0, {int(V)})")
        block[k, :g.shape[0]] = g
        table[k] = g.shape[0]
    return block, table


KEEP_PARTS = {"body": 0, "hand": 1}   # the code grid's columns: column 0 is the body codebook, column 1 the hand codebook


def given_counts(given, given_poses, B):
    """How many given code rows every SUBMITTED clip brings, for `given_keep_block`: G_b for an entry of `given=`, P_b // 4 for an entry of
    `given_poses=`, None for a clip that brings nothing.  Lenient — a malformed entry counts as None; `given_block` / `given_pose_block`
    are what refuse it."""
    def per_clip(x, div):
        if x is None:
            return [None] * B
        if not isinstance(x, (list, tuple)):
            sh = tuple(getattr(x, "shape", ()))
            return [int(sh[1]) // div if len(sh) == 3 else None] * B
        out = [None] * B
        for b, g in enumerate(x[:B]):
            if g is None:
                continue
            sh = tuple(g.shape) if hasattr(g, "shape") else np.shape(g)
            out[b] = int(sh[0]) // div if len(sh) >= 1 else None
        return out
    gc, pc = per_clip(given, 1), per_clip(given_poses, 4)
    return [g if g is not None else p for g, p in zip(gc, pc)]


def given_keep_block(given_keep, counts, rows, order=None, who="given_keep"):
    """The `given_keep=` keyword of the decode entries -> the mask (B, max rows, 2) uint8 in SLOT order that the `_keep` entries take as
    keep_dev (talkshow_hip.h, "kept positions": position (r, j) of a clip is TAKEN from its given rows iff r < G_b and the mask byte is 1,
    and produced otherwise), or None for `given_keep=None` (every given position kept).
    given_keep: one entry per clip in SUBMISSION order — None (keep all of the clip's given rows), "body" (column 0 kept, the hands
    redrawn), "hand" (column 1 kept, the body redrawn) or a (G_b, 2) bool / 0-1 integer array — or one string or one (B, G, 2) block for
    all clips (one string applies to the clips that bring rows).  counts: `given_counts(...)`, every clip's given rows in submission order
    (None: the clip brings nothing); rows: every clip's own code rows H_b; order: sorted slot k holds submitted clip order[k].  Bytes at or
    beyond a clip's G_b are 0 (the pass never reads them).  ValueError naming the SUBMITTED clip for a shape that does not match the clip's
    given rows, an array that is neither bool nor 0 / 1 integers, an unknown string, or an entry on a clip that brings nothing.  Pure host
    code; a device tensor is read back."""
    if given_keep is None:
        return None
    B = len(rows)
    if len(counts) != B:
        raise ValueError(f"{who}: one given-row count per clip ({B}), got {len(counts)}")
    for_all = isinstance(given_keep, str)
    if for_all:
        if given_keep not in KEEP_PARTS:
            raise ValueError(f"{who}: given_keep is None, 'body', 'hand' or a (G, 2) mask, got {given_keep!r}")
        if all(c is None for c in counts):
            raise ValueError(f"{who}: given_keep={given_keep!r} selects from given rows, but clip 0 — like every clip — brings none")
        given_keep = [given_keep if counts[b] is not None else None for b in range(B)]
    if hasattr(given_keep, "detach"):
        given_keep = given_keep.detach().cpu().numpy()
    if isinstance(given_keep, np.ndarray):
        if given_keep.ndim != 3 or given_keep.shape[0] != B or given_keep.shape[2] != 2:
            raise ValueError(f"{who}: one mask for all clips must have shape (B={B}, G, 2), got {tuple(given_keep.shape)}")
        given_keep = list(given_keep)
    if not isinstance(given_keep, (list, tuple)) or len(given_keep) != B:
        raise ValueError(f"{who}: given_keep takes one entry per clip ({B}) — None, 'body', 'hand' or a (G, 2) mask — one string, or one "
                         f"(B, G, 2) block, got {type(given_keep).__name__}" + (f" of {len(given_keep)}" if isinstance(given_keep, (list, tuple)) else ""))
    order = list(range(B)) if order is None else [int(i) for i in order]
    if sorted(order) != list(range(B)):
        raise ValueError(f"{who}: order must be a permutation of the {B} clips")
    mask = np.zeros((B, max(int(h) for h in rows), 2), np.uint8)
    for k, i in enumerate(order):
        m, G = given_keep[i], counts[i]
        if m is not None and G is None:
            raise ValueError(f"{who}: given_keep of clip {i} selects from given rows, but the clip brings none (no given= / given_poses= entry)")
        if G is None:
            continue
        G = min(int(G), mask.shape[1])      # more rows than the clip has: the given helper's error, not this one's
        if m is None:
            mask[k, :G] = 1
        elif isinstance(m, str):
            if m not in KEEP_PARTS:
                raise ValueError(f"{who}: given_keep of clip {i} is None, 'body', 'hand' or a (G, 2) mask, got {m!r}")
            mask[k, :G, KEEP_PARTS[m]] = 1
        else:
            if hasattr(m, "detach"):
                m = m.detach().cpu().numpy()
            m = np.asarray(m)
            if m.shape != (int(counts[i]), 2):
                raise ValueError(f"{who}: given_keep of clip {i} must have shape ({int(counts[i])}, 2), the clip's given rows, got {tuple(m.shape)}")
            if m.dtype.kind not in "biu" or (m.dtype.kind != "b" and m.size and (int(m.min()) < 0 or int(m.max()) > 1)):
                raise ValueError(f"{who}: given_keep of clip {i} must be bool or 0 / 1 integers, got {m.dtype}"
                                 + ("" if m.dtype.kind not in "iu" else f" with the value {int(m[(m < 0) | (m > 1)].flat[0])}"))
            mask[k, :G] = m[:G] != 0
    return mask


def style_block(style, rows, NC, order=None, who="style", ids=None):
    """The `style=` keyword of the decode and scoring entries -> the weight block (B, S, NC) float32 numpy in SLOT order that the `_style`
    entries take as style_dev (after an upload) with style_rows = S, or None for `style=None` (talkshow_hip.h, "speaker style": the
    class-conditioning vector of a code row is the ascending sum of weight * table row over the non-zero weights — an interpolation of
    the speakers' conditioning vectors, NOT a mixture of their distributions).
    style: a list in SUBMISSION order with, per clip, None (the clip's integer id, that is, its one-hot row: `ids` must be given), an
    (NC,) row of weights for the whole clip, or an (H_b, NC) track with one row per code row; or one (NC,) or one (B, NC) array for all
    clips.  rows: every clip's own code rows H_b in submission order; NC: the model's n_classes; order: sorted slot k holds submitted clip
    order[k]; ids: the clips' integer speaker ids in submission order (one for all, or B).  S = 1 if no clip brings a track; otherwise
    S = max rows, per-clip rows are repeated into tracks and a track's rows beyond H_b repeat its last row (the pass does not use them).
    Weights are any finite floats (no sign rule, no sum rule).  ValueError naming the SUBMITTED clip, before anything is launched, for a
    wrong shape, a wrong NC or a non-finite weight (`ts_style_check`).  Pure host code; a device tensor is read back."""
    if style is None:
        return None
    B, NC = len(rows), int(NC)

    def host(x):
        return x.detach().cpu().numpy() if hasattr(x, "detach") else x
    style = host(style)
    if isinstance(style, (list, tuple)) and not any(e is None or np.ndim(host(e)) >= 1 for e in style):
        style = np.asarray(style)      # a plain list of numbers: one row for all clips
    if isinstance(style, np.ndarray):
        if style.ndim == 1:
            style = [style] * B
        elif style.ndim == 2 and style.shape[0] == B:
            style = list(style)
        else:
            raise ValueError(f"{who}: one style array for all clips must have shape (NC={NC},) or (B={B}, NC={NC}), got {tuple(style.shape)} "
                             f"(a track is one entry of a list)")
    if not isinstance(style, (list, tuple)) or len(style) != B:
        raise ValueError(f"{who}: style takes one entry per clip ({B}) — None, an (NC,) row or an (H_b, NC) track — or one (NC,) or (B, NC) "
                         f"array, got {type(style).__name__}" + (f" of {len(style)}" if isinstance(style, (list, tuple)) else ""))
    order = list(range(B)) if order is None else [int(i) for i in order]
    if sorted(order) != list(range(B)):
        raise ValueError(f"{who}: order must be a permutation of the {B} clips")
    if ids is not None and any(e is None for e in style):      # read back only where an entry asks for the clip's id
        ids = np.asarray(host(ids), np.int64).reshape(-1)
        if ids.size == 1 and B > 1:
            ids = np.repeat(ids, B)
    entries = [None] * B
    for i, e in enumerate(style):
        if e is None:
            if ids is None or ids.size != B or not 0 <= int(ids[i]) < NC:
                raise ValueError(f"{who}: style of clip {i} is None — the clip's integer id — but the clip has no id in [0, {NC})")
            e = np.zeros(NC, np.float32)
            e[int(ids[i])] = 1.0
        else:
            e = np.asarray(host(e))
            if e.dtype.kind not in "fiub":
                raise ValueError(f"{who}: style of clip {i} must be numbers, got {e.dtype}")
            if e.ndim not in (1, 2) or (e.ndim == 2 and e.shape[0] != int(rows[i])):
                raise ValueError(f"{who}: style of clip {i} must have shape ({NC},) or ({int(rows[i])}, {NC}), the clip's code rows, got "
                                 f"{tuple(e.shape)}")
            if e.shape[-1] != NC:
                raise ValueError(f"{who}: style of clip {i} has {e.shape[-1]} weights per row, the model has NC = {NC} speakers")
            e = np.ascontiguousarray(e, dtype=np.float32)
            if load().ts_style_check(e.ctypes.data_as(C.POINTER(C.c_float)), int(e.size), NC) != 0:
                raise ValueError(f"{who}: style of clip {i}: " + load().ts_last_error().decode())
        entries[i] = e
    S = max(int(h) for h in rows) if any(e.ndim == 2 for e in entries) else 1
    block = np.zeros((B, S, NC), np.float32)
    for k, i in enumerate(order):
        e = entries[i]
        if e.ndim == 1:
            block[k, :] = e
        else:
            block[k, :e.shape[0]] = e
            block[k, e.shape[0]:] = e[-1]
    return block


def code_bias_block(code_bias, B, V, order=None, who="code_bias", mode=None):
    """The `code_bias=` keyword of the decode entries -> (tables (NB, 2, V) float32, index (B,) int32), both numpy: what the `_bias` entries
    take as bias_dev (after an upload), n_bias = NB and bias_index_host, the index in SLOT order; (None, None) for `code_bias=None`
    (talkshow_hip.h, "code bias": l' = l + b ahead of the sampling rule, row 0 for the body column and row 1 for the hand column; -inf bans
    a code).
    code_bias: one (2, V) array for all clips; or a list in SUBMISSION order with, per clip, None (no table: the clip's bits do not move),
    a (2, V) array, or a dict {"body": (V,), "hand": (V,)} in which a missing key means zeros.  Entries that are the SAME OBJECT share one
    table (NB counts distinct objects).  order: sorted slot k holds submitted clip order[k].  A list of None only gives (None, None).
    mode: the call's draw mode, if the caller wants the scope checked here too (greedy and teacher forced are refused as for a sampling table).
    ValueError naming the SUBMITTED clip, before anything is launched, for a wrong shape, a NaN, a +inf, a finite value beyond 1e30 or a
    column without an allowed code (`ts_code_bias_check`).  Pure host code; a device tensor is read back."""
    if code_bias is None:
        return None, None
    if mode is not None and mode not in (TS_SAMPLE_UNIFORMS, TS_SAMPLE_PHILOX):      # the bias shares the sampling table's scope
        raise ValueError(f"{who}: a code bias is a sampling control: sampling controls need TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX (per-clip "
                         f"greedy is top_k = 1)")
    B, V = int(B), int(V)

    def host(x):
        return x.detach().cpu().numpy() if hasattr(x, "detach") else x
    code_bias = host(code_bias)
    if isinstance(code_bias, (np.ndarray, dict)):
        code_bias = [code_bias] * B
    if not isinstance(code_bias, (list, tuple)) or len(code_bias) != B:
        raise ValueError(f"{who}: code_bias takes one entry per clip ({B}) — None, a (2, V) array or a dict with 'body' / 'hand' rows — or one "
                         f"(2, V) array for all, got {type(code_bias).__name__}" + (f" of {len(code_bias)}" if isinstance(code_bias, (list, tuple)) else ""))
    order = list(range(B)) if order is None else [int(i) for i in order]
    if sorted(order) != list(range(B)):
        raise ValueError(f"{who}: order must be a permutation of the {B} clips")
    tables, seen, index_sub = [], {}, [-1] * B
    for i, e in enumerate(code_bias):
        if e is None:
            continue
        if id(e) in seen:
            index_sub[i] = seen[id(e)]
            continue
        if isinstance(e, dict):
            if not e or any(k not in ("body", "hand") for k in e):
                raise ValueError(f"{who}: code_bias of clip {i}: a dict holds 'body' and / or 'hand' rows, got keys {sorted(map(str, e))}")
            t = np.zeros((2, V), np.float32)
            for j, k in enumerate(("body", "hand")):
                if e.get(k) is not None:
                    r = np.asarray(host(e[k]))
                    if r.dtype.kind not in "fiub" or r.shape != (V,):
                        raise ValueError(f"{who}: code_bias of clip {i}: the '{k}' row must be ({V},) numbers, got {r.dtype} {tuple(r.shape)}")
                    t[j] = r
        else:
            t = np.asarray(host(e))
            if t.dtype.kind not in "fiub" or t.shape != (2, V):
                raise ValueError(f"{who}: code_bias of clip {i} must be a (2, {V}) array of numbers (row 0 body, row 1 hand), got {t.dtype} "
                                 f"{tuple(t.shape)}")
            with np.errstate(over="ignore"):
                t = np.ascontiguousarray(t, dtype=np.float32)
        if load().ts_code_bias_check(t.ctypes.data_as(C.POINTER(C.c_float)), 1, V) != 0:
            msg = load().ts_last_error().decode().replace("ts_code_bias_check: table 0, ", "")
            raise ValueError(f"{who}: code_bias of clip {i}: {msg}")
        seen[id(e)] = index_sub[i] = len(tables)
        tables.append(t)
    if not tables:
        return None, None
    index = np.asarray([index_sub[i] for i in order], np.int32)
    return np.ascontiguousarray(np.stack(tables), dtype=np.float32), index


def repeat_record(rec):
    """One repetition record as (window, presence, frequency): None (off: (0, 0.0, 0.0)), a dict with any of the keys `window`,
    `presence`, `frequency`, or a TUPLE (window, presence, frequency).  A list is never one record: lists hold one record per clip.
    Pure host code."""
    if rec is None:
        return (0, 0.0, 0.0)
    if isinstance(rec, dict):
        unknown = set(rec) - {"window", "presence", "frequency"}
        if unknown:
            raise ValueError(f"repetition record: unknown keys {sorted(map(str, unknown))} (window, presence, frequency)")
        rec = (rec.get("window", 0), rec.get("presence", 0.0), rec.get("frequency", 0.0))
    if isinstance(rec, tuple) and len(rec) == 3:
        w, p, f = rec
        try:      # inf, NaN, a string, None: refused like a fraction, as a ValueError the caller can name the clip in
            whole = not isinstance(w, bool) and int(w) == w
        except (TypeError, ValueError, OverflowError):
            whole = False
        if not whole:
            raise ValueError(f"a repetition record's window is a whole number of code rows, got {w!r}")
        try:
            return (int(w), float(p), float(f))
        except (TypeError, ValueError):
            raise ValueError(f"a repetition record's presence and frequency are numbers, got {p!r} and {f!r}") from None
    raise ValueError(f"a repetition record is None, a dict or a tuple (window, presence, frequency), got {rec!r}")


def repeat_table(repeat, B, V, order=None, who="repeat", mode=None):
    """The `repeat=` keyword of the decode entries -> (array of B `ts_repeat` records in SLOT order, B): what the `_repeat` entries take as
    rep_host and n_rep; (None, 0) for `repeat=None` (talkshow_hip.h, "repetition penalty": a code the clip produced in the last `window`
    rows of a column loses presence + frequency * count ahead of the sampling rule).
    repeat: None, a dict or a tuple (window, presence, frequency) — ONE record for all clips — or a LIST in SUBMISSION order with one such
    entry per clip.  A single record written as a list is refused with a message that says so.  order: sorted slot k holds submitted clip
    order[k].  mode: the call's draw mode, if the caller wants the scope checked here too (greedy and teacher forced are refused as for a
    sampling table).  ValueError naming the SUBMITTED clip, before anything is launched, for a window outside [0, 64], a NaN, an
    infinity or a value beyond 1e30 (`ts_repeat_check`).  Pure host code."""
    if repeat is None:
        return None, 0
    if mode is not None and mode not in (TS_SAMPLE_UNIFORMS, TS_SAMPLE_PHILOX):      # the penalty shares the sampling table's scope
        raise ValueError(f"{who}: a repetition penalty is a sampling control: sampling controls need TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX "
                         f"(per-clip greedy is top_k = 1)")
    B = int(B)
    if isinstance(repeat, (dict, tuple)):
        recs = [repeat] * B
    elif isinstance(repeat, list):
        if repeat and all(isinstance(r, (int, float)) for r in repeat):
            raise ValueError(f"{who}: repeat={repeat!r}: a list holds one record per clip; write one record for all clips as a tuple "
                             f"(window, presence, frequency)")
        if len(repeat) != B:
            raise ValueError(f"{who}: repeat must hold one record or one per clip ({B}), got {len(repeat)}")
        recs = repeat
    else:
        raise ValueError(f"{who}: repeat must be None, a dict, a tuple (window, presence, frequency) or a list of one record per clip, got {repeat!r}")
    order = list(range(B)) if order is None else [int(i) for i in order]
    if sorted(order) != list(range(B)):
        raise ValueError(f"{who}: order must be a permutation of the {B} clips")
    one = (TsRepeat * 1)()
    arr = (TsRepeat * B)()
    checked = {}
    for i, r in enumerate(recs):
        try:
            w, p, f = repeat_record(r)
        except ValueError as e:
            raise ValueError(f"{who}: repeat of clip {i}: {e}") from None
        if (w, p, f) not in checked:
            if not -2 ** 31 <= w < 2 ** 31:
                raise ValueError(f"{who}: repeat of clip {i}: window out of range")
            one[0].window, one[0].presence, one[0].frequency, one[0].reserved = w, p, f, 0
            if load().ts_repeat_check(one, 1, int(V)) != 0:
                msg = load().ts_last_error().decode().replace("ts_repeat_check: clip 0: ", "")
                raise ValueError(f"{who}: repeat of clip {i}: {msg}")
            checked[(w, p, f)] = True
    for k, i in enumerate(order):
        w, p, f = repeat_record(recs[i])
        arr[k].window, arr[k].presence, arr[k].frequency, arr[k].reserved = w, p, f, 0
    return arr, B


GUIDE_MAX_SCALE = 1e4


def guide_style(v, rows, NC, who, name):
    """One guide entry's "style" as a validated float32 array: an (NC,) row or a (rows, NC) track of finite weights (`ts_style_check`).
    ValueError naming clip `name`.  The one place these messages are made.  Pure host code; a device tensor is read back."""
    v = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    if v.dtype.kind not in "fiub" or v.ndim not in (1, 2) or (v.ndim == 2 and v.shape[0] != int(rows)) or v.shape[-1] != int(NC):
        raise ValueError(f"{who}: guide of clip {name}: the style must have shape ({int(NC)},) or ({int(rows)}, {int(NC)}), got {v.dtype} {tuple(v.shape)}")
    v = np.ascontiguousarray(v, dtype=np.float32)
    if load().ts_style_check(v.ctypes.data_as(C.POINTER(C.c_float)), int(v.size), int(NC)) != 0:
        raise ValueError(f"{who}: guide of clip {name}: style: " + load().ts_last_error().decode())
    return v


def guide_entries(guide, B, who="guide", audio_key="mfcc", mode=None, n_classes=None, rows=None):
    """The `guide=` keyword of the decode entries -> a list of B entries in SUBMISSION order, each None or a dict {"scale": float, "audio":
    the entry's `audio_key` value or None, "id": int or None, "style": row / track or None}; None for `guide=None` or a list of None only
    (talkshow_hip.h, "guidance": the clip is decoded under its own conditioning and at every position its logits are pushed away from, or
    toward, those the same code history gets under a second conditioning — l' = l + scale * (l - l_q)).
    guide: one dict for all clips, or a list with, per clip, None or a dict with the keys "scale" (required) and, each optional and None
    meaning "the clip's own", `audio_key` ("mfcc", "wav" or "aud_rows": the second conditioning's audio, of the clip's own length), "id"
    (in [0, n_classes) where n_classes is given) and "style" (validated here — shape and finite weights, `guide_style` — where rows, every
    clip's own code rows in submission order, and n_classes are given; the entry then holds the float32 array).  mode: the call's draw mode, if the caller wants the scope checked here too.  Shapes of audio and style are the call
    site's to check.  ValueError naming the SUBMITTED clip for a wrong key, a scale that is no number, a NaN, an infinity or |scale| > 1e4.
    Pure host code."""
    if guide is None:
        return None
    B = int(B)
    if isinstance(guide, dict):
        guide = [guide] * B
    if not isinstance(guide, (list, tuple)) or len(guide) != B:
        raise ValueError(f"{who}: guide takes one dict for all clips or a list with None or a dict per clip ({B}), got {type(guide).__name__}" +
                         (f" of {len(guide)}" if isinstance(guide, (list, tuple)) else ""))
    keys = ("scale", audio_key, "id", "style")
    out = [None] * B
    for i, e in enumerate(guide):
        if e is None:
            continue
        if not isinstance(e, dict):
            raise ValueError(f"{who}: guide of clip {i} must be None or a dict with the keys {keys}, got {type(e).__name__}")
        unknown = [k for k in e if k not in keys]
        if unknown:
            raise ValueError(f"{who}: guide of clip {i}: unknown keys {sorted(map(str, unknown))} (the keys are {keys})")
        if "scale" not in e:
            raise ValueError(f"{who}: guide of clip {i} needs a scale")
        try:
            if isinstance(e["scale"], bool):
                raise TypeError
            with np.errstate(over="ignore"):
                scale = float(np.float32(e["scale"]))
        except (TypeError, ValueError):
            raise ValueError(f"{who}: guide of clip {i}: the scale is a number, got {e['scale']!r}") from None
        if np.isnan(scale):
            raise ValueError(f"{who}: guide of clip {i}: the scale is NaN")
        if np.isinf(scale):
            raise ValueError(f"{who}: guide of clip {i}: the scale is infinite")
        if abs(scale) > np.float32(GUIDE_MAX_SCALE):
            raise ValueError(f"{who}: guide of clip {i}: the scale exceeds 1e4 in magnitude")
        ident = e.get("id")
        if ident is not None:
            try:
                if isinstance(ident, bool) or int(ident) != ident:
                    raise TypeError
                ident = int(ident)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: guide of clip {i}: the id is a whole number, got {e.get('id')!r}") from None
            if n_classes is not None and not 0 <= ident < int(n_classes):
                raise ValueError(f"{who}: guide of clip {i}: the id {ident} is outside [0, {int(n_classes)})")
        style = e.get("style")
        if style is not None and rows is not None and n_classes is not None:
            style = guide_style(style, rows[i], n_classes, who, i)
        out[i] = {"scale": scale, "audio": e.get(audio_key), "id": ident, "style": style}
    if all(e is None for e in out):
        return None
    if mode is not None and mode not in (TS_SAMPLE_UNIFORMS, TS_SAMPLE_PHILOX):      # guidance shares the sampling table's scope
        raise ValueError(f"{who}: guidance is a sampling control: sampling controls need TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX (per-clip "
                         f"greedy is top_k = 1)")
    return out


def guide_layout(order, entries):
    """The slots of a guided pass: order (sorted slot k holds submitted clip order[k]) and `guide_entries`' list -> (src, shadow, guide,
    scale): the pass has len(src) slots; slot s copies every per-clip entry of ORIGINAL slot src[s]; shadow[s] says whether it is the
    shadow of the slot before it; guide (int32) / scale (float32) are the guided entries' tables.  Every shadow sits directly behind
    its primary, so the non-increasing length order holds and both are active in the same chunks.  Pure host code."""
    src, shadow, guide, scale = [], [], [], []
    for k, i in enumerate(order):
        e = entries[int(i)]
        src.append(k), shadow.append(False), guide.append(-1), scale.append(0.0)
        if e is not None:
            guide[-1], scale[-1] = len(src), e["scale"]
            src.append(k), shadow.append(True), guide.append(-1), scale.append(0.0)
    return src, shadow, np.asarray(guide, np.int32), np.asarray(scale, np.float32)


def expand_records(arr, n, src):
    """A ctypes array of n records (a sampling or repetition table in slot order) re-indexed for a guided pass: slot s takes record src[s].
    A table of one record for all clips stays as it is."""
    if arr is None or int(n) == 1:
        return arr, n
    out = (type(arr[0]) * len(src))()
    for s, k in enumerate(src):
        C.memmove(C.byref(out, s * C.sizeof(out[0])), C.byref(arr, int(k) * C.sizeof(arr[0])), C.sizeof(out[0]))
    return out, len(src)


def guide_style_block(sblock, src, shadow, entries, rows, NC, ids, who="guide", names=None):
    """The style block of a guided pass: sblock = `style_block`'s (B, S, NC) block of the clips themselves in slot order, or None (the
    pass runs on integer ids); src / shadow from `guide_layout`; entries[k] the guide entry of ORIGINAL slot k (or None); rows[k] its code
    rows; ids (B,) the clips' integer ids in slot order (numpy; read only where a block has to be made of them); names[k] the submitted
    index the messages name -> the (len(src), S', NC) block in which a shadow's rows are its "style" (an (NC,) row or a (rows[k], NC)
    track), else the one-hot row of its "id", else its primary's rows; None if sblock is None and no shadow brings a style (the ids
    carry every conditioning, the shadows' included).  ValueError naming the clip for a wrong shape or a non-finite weight."""
    NC = int(NC)
    names = list(range(len(rows))) if names is None else names
    styles = {}
    for s, k in enumerate(src):
        e = entries[k] if shadow[s] else None
        if e is None or e["style"] is None:
            continue
        styles[s] = guide_style(e["style"], rows[k], NC, who, names[k])      # (validated by `guide_entries` already where it had the rows)
    if sblock is None and not styles:
        return None
    if sblock is None:
        ids = np.asarray(ids, np.int64).reshape(-1)
        sblock = np.zeros((len(rows), 1, NC), np.float32)
        sblock[np.arange(len(rows)), 0, ids] = 1.0
    block = np.ascontiguousarray(sblock[np.asarray(src, np.int64)])
    if block.shape[1] == 1 and any(v.ndim == 2 for v in styles.values()):
        block = np.ascontiguousarray(np.repeat(block, max(int(h) for h in rows), axis=1))
    for s, k in enumerate(src):
        if not shadow[s]:
            continue
        if s in styles:
            v = styles[s]
            if v.ndim == 1:
                block[s, :] = v
            else:
                block[s, :v.shape[0]] = v
                block[s, v.shape[0]:] = v[-1]
        elif entries[k]["id"] is not None:
            block[s, :] = 0.0
            block[s, :, entries[k]["id"]] = 1.0
    return block


def guide_expand(src, shadow, ctl=(None, 0), given=(None, None), poses=(None, None), keep=None, bias=(None, None), repeat=(None, 0)):
    """The validated per-clip blocks of a pass (slot order) re-indexed to the slots of the guided pass (`guide_layout`): slot s takes the
    entry of original slot src[s]; a shadow brings no given rows, no poses and no bias table (its sampling and repetition records are
    its primary's and are never read).  Returns (ctl, given, poses, keep, bias, repeat) in the forms they came in.  Pure host code
    (a pose block that is a device tensor is re-indexed on its device)."""
    sidx, shadows = np.asarray(src, np.int64), np.asarray(shadow, bool)
    ctl, repeat = expand_records(ctl[0], ctl[1], src), expand_records(repeat[0], repeat[1], src)
    gblock, gtable = given
    if gblock is not None:
        given = (gblock[sidx], np.where(shadows, 0, gtable[sidx]).astype(np.int32))
    pblock, ptable = poses
    if pblock is not None:
        if hasattr(pblock, "index_select"):
            import torch
            pblock = pblock.index_select(0, torch.as_tensor(sidx, device=pblock.device))
        else:
            pblock = pblock[sidx]
        poses = (pblock, np.where(shadows, 0, ptable[sidx]).astype(np.int32))
    keep = None if keep is None else np.ascontiguousarray(keep[sidx])
    btab, bidx = bias
    if btab is not None:
        bias = (btab, np.where(shadows, -1, bidx[sidx]).astype(np.int32))
    return ctl, given, poses, keep, bias, repeat


def guide_check(guide, scale, lens=None):
    """`ts_guide_check` on host tables: ValueError with the library's message (it names the slot).  Pure host code."""
    guide = np.ascontiguousarray(guide, np.int32)
    scale = np.ascontiguousarray(scale, np.float32)
    i32p = C.POINTER(C.c_int32)
    lens_p = None if lens is None else np.ascontiguousarray(lens, np.int32)
    if load().ts_guide_check(guide.ctypes.data_as(i32p), scale.ctypes.data_as(_fp), None if lens_p is None else lens_p.ctypes.data_as(i32p),
                             int(guide.size)) != 0:
        raise ValueError(load().ts_last_error().decode())


def given_pose_block(given_poses, rows, order=None, who="given_poses", width=129):
    """The `given_poses=` keyword of the decode entries -> (block (B, P_max, width) float32, table (B,) int32 numpy), both in SLOT order: what
    `ts_body_pixel_infer_mixed_poses` takes as given_poses_dev and pose_lens_host (talkshow_hip.h, "given poses").
    given_poses: a list in SUBMISSION order with None (nothing given) or a (P_b, width) float array per clip, or one (B, P, width) block;
    rows: every clip's own code rows H_b in submission order; order: sorted slot k holds submitted clip order[k] (None: the submitted order).
    The rule of `sampling.given_pose_rows`: P_b = 0, or P_b >= 4 with P_b // 4 <= H_b.  Frames of the block at or beyond a clip's P_b are 0
    (the pass never reads them).  ValueError naming the SUBMITTED clip for a bad shape, a non-float array, 1 <= P_b <= 3 or too many frames.
    The block is a numpy array when every entry lives on the host; with a device tensor among them it is a torch tensor on that device and no
    entry is read back.  Pure host code: the library is not loaded."""
    B = len(rows)
    if hasattr(given_poses, "shape") and not isinstance(given_poses, (list, tuple)):
        if len(given_poses.shape) != 3 or given_poses.shape[0] != B or given_poses.shape[2] != width:
            raise ValueError(f"{who}: one block for all clips must have shape (B={B}, P, {width}), got {tuple(given_poses.shape)}")
        given_poses = [given_poses[b] for b in range(B)]
    if not isinstance(given_poses, (list, tuple)) or len(given_poses) != B:
        raise ValueError(f"{who}: one entry per clip ({B}) — None or a (P, {width}) float array — or one (B, P, {width}) block, got "
                         f"{type(given_poses).__name__}" + (f" of {len(given_poses)}" if isinstance(given_poses, (list, tuple)) else ""))
    order = list(range(B)) if order is None else [int(i) for i in order]
    if sorted(order) != list(range(B)):
        raise ValueError(f"{who}: order must be a permutation of the {B} clips")
    table = np.zeros(B, np.int32)
    slots, device = [None] * B, None
    for k, i in enumerate(order):
        g = given_poses[i]
        if g is None:
            continue
        if not hasattr(g, "detach"):
            g = np.asarray(g)
        if len(g.shape) != 2 or g.shape[1] != width:
            raise ValueError(f"{who}: given poses of clip {i} must have shape (P, {width}), got {tuple(g.shape)}")
        if not (g.dtype.is_floating_point if hasattr(g, "detach") else g.dtype.kind == "f"):
            raise ValueError(f"{who}: given poses of clip {i} must be floats, got {g.dtype}")
        P = int(g.shape[0])
        if 1 <= P <= 3:
            raise ValueError(f"{who}: clip {i} brings {P} given pose frames; one code row needs 4 (or none)")
        if P // 4 > int(rows[i]):
            raise ValueError(f"{who}: clip {i} brings {P} given pose frames = {P // 4} code rows but has {int(rows[i])} code rows of its own")
        if hasattr(g, "detach") and g.is_cuda and device is None:
            device = g.device
        slots[k], table[k] = g, P
    P_max = int(table.max()) if B else 0
    if device is None:
        block = np.zeros((B, P_max, width), np.float32)
        for k, g in enumerate(slots):
            if g is not None and table[k]:
                block[k, :table[k]] = g.detach().numpy() if hasattr(g, "detach") else g
        return block, table
    block = torch.zeros((B, P_max, width), dtype=torch.float32, device=device)
    for k, g in enumerate(slots):
        if g is not None and table[k]:
            block[k, :int(table[k])] = torch.as_tensor(g, dtype=torch.float32).to(device)
    return block, table


def given_kinds_check(given, given_poses, B, who="given"):
    """A clip brings `given` rows or `given_poses` frames, never both: ValueError naming the first clip with both.  Entries that are not
    per-clip lists (one block for all clips) count for every clip.  Pure host code."""
    if given is None or given_poses is None:
        return
    has_g = [g is not None for g in given] if isinstance(given, (list, tuple)) else [True] * B
    has_p = [g is not None for g in given_poses] if isinstance(given_poses, (list, tuple)) else [True] * B
    for b, (g, p) in enumerate(zip(has_g, has_p)):
        if g and p:
            raise ValueError(f"{who}: clip {b} brings both given code rows and given poses; a clip brings one kind")


def score_codes_shape(codes_shape, B, H):
    """`score` / `score_batch` take the codes of the pass they score: (B, H, 2).  ValueError otherwise; pure host code."""
    if tuple(codes_shape) != (int(B), int(H), 2):
        raise ValueError(f"score: codes must have shape (B, H, 2) = ({int(B)}, {int(H)}, 2), got {tuple(codes_shape)}")


def pack_state_dict(sd):
    """{name: tensor/ndarray} -> (ts_tensor array, n, keepalive).  Non-float entries are passed with data=NULL."""
    items = list(sd.items())
    arr = (TsTensor * len(items))()
    keep = []
    for k, (name, v) in enumerate(items):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.asarray(v)
        bname = name.encode()
        keep.append(bname)
        arr[k].name = bname
        arr[k].ndim = min(v.ndim, 4)
        for d in range(min(v.ndim, 4)):
            arr[k].shape[d] = v.shape[d]
        if v.dtype == np.float32 and v.ndim <= 4:
            v = np.ascontiguousarray(v)
            keep.append(v)
            arr[k].data = fptr(v)
        else:
            arr[k].data = None
    return arr, len(items), keep


def create_streams(n, device_index=None, cus=None):
    """n library-created HIP streams wrapped as torch ExternalStreams (created back to back -> distinct HW queues).

    cus=(first, count) restricts their kernels to that range of compute units (ts_stream_create_cus)."""
    ctx = context(device_index)
    out = []
    for _ in range(n):
        h = _vp()
        if cus is None:
            check(load().ts_stream_create(ctx, C.byref(h)))
        else:
            check(load().ts_stream_create_cus(ctx, int(cus[0]), int(cus[1]), C.byref(h)))
        out.append(torch.cuda.ExternalStream(h.value, device=torch.device("cuda", device_index if device_index is not None
                                                                              else torch.cuda.current_device())))
    return out


_contexts = {}


def context(device_index=None):
    """One ts_ctx per HIP device per process."""
    if not torch.cuda.is_available():
        raise RuntimeError("talkshow_amd needs a HIP device (MI355X / gfx950); torch.cuda.is_available() is False. "
                           "There is no CPU path.")
    if device_index is None:
        device_index = torch.cuda.current_device()
    if device_index not in _contexts:
        lib = load()
        h = _vp()
        check(lib.ts_ctx_create(int(device_index), C.byref(h)))
        _contexts[device_index] = h
    return _contexts[device_index]
