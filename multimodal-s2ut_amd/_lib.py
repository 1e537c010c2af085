"""ctypes binding of libmms2ut_hip.so (the C-ABI declared in include/mms2ut.h).

The product path has no CPU fallback: if the library is missing or a call fails, this raises.
"""
import ctypes as C
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMS2UT_LIB") or os.path.join(HERE, "lib", "libmms2ut_hip.so")  # override: A/B builds

vp, i32, i64, u64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float

EPI_F16, EPI_RELU_DROP, EPI_DROP_RESID, EPI_F32, EPI_GATE, EPI_RELU_DROP_BWD, EPI_F16_ACC, EPI_GELU_DROP, \
    EPI_GELU_DROP_BWD = range(9)


class GemmArgs(C.Structure):
    _fields_ = [
        ("A", vp), ("B", vp), ("C", vp),
        ("M", i32), ("N", i32), ("K", i32),
        ("a_kcontig", i32), ("b_kcontig", i32),
        ("lda", i64), ("ldb", i64), ("ldc", i64),
        ("batch", i32), ("bdiv", i32),
        ("sA1", i64), ("sA2", i64), ("sB1", i64), ("sB2", i64), ("sC1", i64), ("sC2", i64),
        ("splitk", i32),
        ("sCsplit", i64),
        ("epi", i32),
        ("alpha", f32),
        ("bias", vp), ("aux", vp),
        ("ldaux", i64), ("sX1", i64), ("sX2", i64),
        ("out2", vp),
        ("ldo2", i64),
        ("dropout_p", f32),
        ("seed", u64), ("offset", u64),
        ("ld_rng", i64),
        ("rowsum", vp), ("ld_rowsum", i64),
        ("splitk_ws", vp), ("splitk_ws_floats", i64),
    ]


def _packer(st):
    """struct.Struct with the C layout of a ctypes Structure (native alignment, same field order):
    packing all fields in one call costs ~2 us where ~45 ctypes attribute stores cost ~10 us, and
    the training step issues a few hundred GEMMs per step from Python."""
    code = {vp: "P", i32: "i", i64: "q", f32: "f", u64: "Q"}
    fmt = "@" + "".join(code[t] for _, t in st._fields_)
    tail = C.sizeof(st) - struct.calcsize(fmt)          # the C struct's trailing alignment padding
    S = struct.Struct(fmt + (f"{tail}x" if tail > 0 else ""))
    assert S.size == C.sizeof(st), (S.size, C.sizeof(st))
    return S


# mms2ut_gemm_args as one bytes object: fields in GemmArgs._fields_ order, null pointers as 0
GEMM_ARGS = _packer(GemmArgs)


class AttnArgs(C.Structure):
    _fields_ = [
        ("q", vp), ("k", vp), ("v", vp), ("o", vp),
        ("ldq", i64), ("ldk", i64), ("ldv", i64), ("ldo", i64),
        ("sqb", i64), ("skb", i64), ("svb", i64), ("sob", i64),
        ("B", i32), ("H", i32), ("Tq", i32), ("Tk", i32), ("hd", i32),
        ("key_len", vp),
        ("causal", i32),
        ("scale", f32),
        ("p", f32),
        ("seed", u64), ("offset", u64),
        ("lse", vp),
    ]


ATTN_ARGS = _packer(AttnArgs)


class AttnFwdPlan(C.Structure):
    """mms2ut_attn_fwd_plan: what mms2ut_mha_varlen_fwd would launch."""
    _fields_ = [(n, i32) for n in ("nw", "short_k", "grid_x", "grid_y")]


class AttnBwdPlan(C.Structure):
    """mms2ut_attn_bwd_plan: what mms2ut_mha_varlen_bwd would launch."""
    _fields_ = [(n, i32) for n in ("fused", "nkc", "kv16", "rows_prep", "grid", "rounds")]


LAYER_ENC, LAYER_DEC = 0, 1
(SLOT_M1, SLOT_R1, SLOT_H1, SLOT_QKV, SLOT_LSE_SA, SLOT_O, SLOT_XA, SLOT_M2, SLOT_R2, SLOT_H2, SLOT_Q, SLOT_LSE_CA,
 SLOT_CO, SLOT_XB, SLOT_M3, SLOT_R3, SLOT_H3, SLOT_F1, SLOT_OUT, LAYER_NSLOT) = range(20)


class LayerArgs(C.Structure):
    """mms2ut_layer (include/mms2ut.h): one pre-LN transformer layer."""
    _fields_ = [("kind", i32), ("B", i32), ("T", i32), ("Tk", i32), ("d", i32), ("H", i32), ("F", i32),
                ("eps", f32), ("self_len", vp), ("cross_len", vp)] + \
        [(n, vp) for n in ("ln1_g", "ln1_b", "w_qkv", "b_qkv", "w_o", "b_o", "ln2_g", "ln2_b", "w_cq", "b_cq",
                           "w_co", "b_co", "kv")] + [("ld_kv", i64)] + \
        [(n, vp) for n in ("ln3_g", "ln3_b", "w_fc1", "b_fc1", "w_fc2", "b_fc2",
                           "wt_qkv", "wt_o", "wt_cq", "wt_co", "wt_fc1", "wt_fc2",
                           "g_ln1", "g_w_qkv", "g_b_qkv", "g_w_o", "g_b_o", "g_ln2", "g_w_cq", "g_b_cq",
                           "g_w_co", "g_b_co", "g_ln3", "g_w_fc1", "g_b_fc1", "g_w_fc2", "g_b_fc2")] + \
        [("p_drop", f32), ("p_attn", f32), ("p_act", f32), ("seed", u64)] + \
        [(n, u64) for n in ("off_sa_attn", "off_sa_res", "off_ca_attn", "off_ca_res", "off_act", "off_ffn_res")] + \
        [("x", vp), ("saved", vp)]


CONV_MAX = 4   # include/mms2ut.h MMS_CONV_MAX


class ConvArgs(C.Structure):
    """mms2ut_conv1d_glu (include/mms2ut.h): the Conv1d subsampler."""
    _fields_ = [("B", i32), ("T", i32), ("C", i32), ("nlayers", i32), ("k", i32 * CONV_MAX), ("cout", i32 * CONV_MAX)] + \
        [(n, vp * CONV_MAX) for n in ("w", "b", "wt", "g_w", "g_b")] + [("x", vp), ("saved", vp)]


class FusionArgs(C.Structure):
    """mms2ut_gated_fusion (include/mms2ut.h): the fusion tail."""
    _fields_ = [(n, i32) for n in ("B", "Te", "Ti", "Di", "d", "extra", "gate", "image_pre_norm")] + \
        [(n, f32) for n in ("eps", "p_img", "p_txt", "p_attn")] + [(n, u64) for n in ("seed", "off_img", "off_txt", "off_attn")] + \
        [("key_mask", vp), ("ld_mask", i64)] + \
        [(n, vp) for n in ("ln_g", "ln_b", "wq", "bq", "wkv", "bkv", "bias_kv", "wo", "bo", "wg", "bg",
                           "g_ln", "g_wq", "g_bq", "g_wkv", "g_bkv", "g_bias_kv", "g_wo", "g_bo", "g_wg", "g_bg",
                           "wt_q", "wt_kv", "wt_o", "wt_g", "text", "img", "saved")]


OP_LAYER, OP_CONV1D_GLU, OP_GATED_FUSION = range(3)   # include/mms2ut.h MMS_OP_*


class WgradArgs(C.Structure):
    """mms2ut_wgrad (include/mms2ut.h): one problem of a grouped weight-gradient launch."""
    _fields_ = [("dy", vp), ("lddy", i64), ("x", vp), ("ldx", i64), ("dW", vp), ("db", vp), ("N", i32), ("K", i32)]


class LayerGradArgs(C.Structure):
    """mms2ut_layer_grad (include/mms2ut.h)."""
    _fields_ = [("dy", vp), ("dy_drop", vp), ("emit_p", f32), ("emit_seed", u64), ("emit_offset", u64),
                ("dkv", vp), ("ld_dkv", i64), ("scratch", vp), ("main_ws", vp), ("main_ws_floats", i64),
                ("side_ws", vp), ("side_ws_floats", i64), ("side_blocks", i32)]


LAYER_GRAD_ARGS = _packer(LayerGradArgs)

VOC_CIN_CHUNK, VOC_MAX_SPAN = 64, 64                     # include/mms2ut.h MMS_VOC_*
VOC_ACC_NONE, VOC_ACC_SET, VOC_ACC_ADD = range(3)


class Conv1dTmArgs(C.Structure):
    """mms2ut_conv1d_tm_args (include/mms2ut.h): one implicit-GEMM Conv1d launch of the vocoder."""
    _fields_ = [("x", vp), ("ldx", i64), ("T_in", i32), ("Cin", i32), ("w", vp), ("w_phase", i64), ("bias", vp),
                ("y", vp), ("ldy", i64), ("T_out", i32), ("Cout", i32), ("taps", i32), ("dil", i32), ("pad", i32),
                ("nq", i32), ("phases", i32), ("ostride", i32), ("ooff", i32), ("in_act", i32), ("in_slope", f32),
                ("res", vp), ("ldres", i64), ("acc", i32), ("scale", f32), ("out_act", i32), ("out_slope", f32)]


CONV1D_TM_ARGS = _packer(Conv1dTmArgs)

VOC_MAX_STAGES, VOC_MAX_RESBLOCKS, VOC_MAX_DILS = 8, 4, 4   # include/mms2ut.h MMS_VOC_MAX_*


class VocConv(C.Structure):
    _fields_ = [("w", vp), ("b", vp), ("k", i32), ("dil", i32)]


class VocUp(C.Structure):
    _fields_ = [("w", vp), ("b", vp), ("k", i32), ("u", i32), ("cout", i32)]


class HifiGan(C.Structure):
    """mms2ut_hifigan (include/mms2ut.h): the generator's weights for mms2ut_hifigan_fwd."""
    _fields_ = [("dict", vp), ("n_embed", i32), ("D", i32), ("C0", i32), ("n_stages", i32), ("nk", i32),
                ("nd", i32 * VOC_MAX_RESBLOCKS), ("pre", VocConv), ("ups", VocUp * VOC_MAX_STAGES),
                ("c1", VocConv * VOC_MAX_DILS * VOC_MAX_RESBLOCKS * VOC_MAX_STAGES),
                ("c2", VocConv * VOC_MAX_DILS * VOC_MAX_RESBLOCKS * VOC_MAX_STAGES),
                ("post_w", vp), ("post_b", f32), ("post_k", i32), ("slope", f32), ("post_slope", f32)]


ASR_STAT_WS_DOUBLES = 128                                # include/mms2ut.h MMS_ASR_*
ASR_CONV0_MAX_C, ASR_CONV0_MAX_K, ASR_CONV0_MAX_S, ASR_CONV_MAX_ROWS, ASR_LN_MAX_C = 512, 16, 16, 264, 1024


class AsrConvArgs(C.Structure):
    """mms2ut_asr_conv_args (include/mms2ut.h): one strided / grouped implicit-GEMM Conv1d launch."""
    _fields_ = [("x", vp), ("ldx", i64), ("T_in", i32), ("Cin", i32), ("w", vp), ("w_group", i64), ("bias", vp),
                ("y", vp), ("ldy", i64), ("T_out", i32), ("Cout", i32), ("taps", i32), ("stride", i32), ("pad", i32),
                ("groups", i32), ("res", vp), ("ldres", i64), ("gelu", i32)]


ASR_CONV_ARGS = _packer(AsrConvArgs)
HUBERT_GN_PARTS, KMEANS_LO_SCALE = 256, 2048              # include/mms2ut.h MMS_HUBERT_GN_PARTS, MMS_KMEANS_LO_SCALE
KMEANS_TOPK_MAX, UNITS_BEAM_MAX_CAND = 32, 2048           # include/mms2ut.h MMS_KMEANS_TOPK_MAX, MMS_UNITS_BEAM_MAX_CAND

KMEANS_STATE, KMEANS_PP_MAX_TRIALS, KMEANS_PP_ROWS = 8, 16, 16   # include/mms2ut.h MMS_KMEANS_STATE, MMS_KMEANS_PP_*


class KMeansStepArgs(C.Structure):
    """mms2ut_kmeans_step_args (include/mms2ut.h): the buffers of one mini-batch k-means step."""
    _fields_ = [("X", vp), ("ldx", i64), ("N", i64), ("norms", vp), ("R", i32), ("d", i32), ("K", i32), ("chunk", i32)] + \
        [(n, vp) for n in ("C", "counts", "c_hi", "c_lo", "cnorm", "Xb", "xnorm_b", "pscore", "pidx", "code", "best",
                           "partials", "sums", "cnt", "bad", "state")] + [("alpha", C.c_double), ("max_no_improvement", i32)]


VISION_TILE_BYTES, VISION_MAX_SIDE = 49152, 65535         # include/mms2ut.h MMS_VISION_*
ROLLOUT_MAX_T = 640                                       # include/mms2ut.h MMS_ROLLOUT_MAX_T
SCORE_MAX_LEN = 4096                                      # include/mms2ut.h MMS_SCORE_MAX_LEN


class ImageDesc(C.Structure):
    """mms2ut_image_desc (include/mms2ut.h): one image of a mms2ut_vision_patches launch."""
    _fields_ = [("src", i64), ("w", C.c_int32), ("h", C.c_int32)] + \
        [(n, C.c_int32) for n in ("hb", "hk", "hn", "vb", "vk", "vn")]


# name -> (restype, argtypes); every symbol include/mms2ut.h declares
SIGNATURES = {
    "mms2ut_last_error": (C.c_char_p, []),
    "mms2ut_version": (i32, []),
    "mms2ut_stream_create": (i32, [i32, vp]),
    "mms2ut_stream_destroy": (i32, [vp]),
    "mms2ut_event_create": (i32, [vp]),
    "mms2ut_event_record": (i32, [vp, vp]),
    "mms2ut_event_wait": (i32, [vp, vp]),
    "mms2ut_event_destroy": (i32, [vp]),
    "mms2ut_gemm_f16": (i32, [vp, vp]),   # GEMM_ARGS.pack(...) bytes or C.byref(GemmArgs)
    "mms2ut_gemm_set_tall": (i32, [i32]),
    "mms2ut_gemm_set_skinny": (i32, [i32]),
    "mms2ut_gemm_skinny_debug": (i32, [i32, vp]),
    "mms2ut_gemm_set_epilogue": (i32, [i32]),
    "mms2ut_wgrad_group": (i32, [vp, i32, i64, i32, vp]),
    "mms2ut_wgrad_flush": (i32, [vp]),
    "mms2ut_profile_begin": (i32, [i32]),
    "mms2ut_profile_end": (i32, [C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "mms2ut_profile_bytes": (i32, [C.POINTER(C.c_double)]),
    "mms2ut_profile_launches": (i32, [C.c_void_p, C.c_void_p, C.c_void_p, i32]),
    "mms2ut_profile_shapes": (i32, [C.c_void_p, i32]),
    "mms2ut_profile_stamps": (i32, [vp, C.c_long]),
    "mms2ut_profile_blocks": (i32, [C.c_void_p, i32]),
    "mms2ut_wallclock_khz": (i32, [C.POINTER(C.c_int)]),
    "mms2ut_grad_norm_check": (i32, [vp, i32, i32, vp, i32, vp]),
    "mms2ut_ctc_workspace_floats": (i32, [i32, i32, i32, C.POINTER(C.c_int64)]),
    "mms2ut_ctc_loss_fwd": (i32, [vp, i64, i32, i32, i32, vp, i64, i32, vp, vp, i32, i32, vp, vp, vp]),
    "mms2ut_ctc_loss_bwd": (i32, [vp, i64, i32, i32, i32, vp, i64, i32, vp, vp, i32, vp, vp, vp, i64, vp]),
    "mms2ut_scale_f16": (i32, [vp, i64, f32, vp]),
    "mms2ut_accum_f16_f32": (i32, [vp, vp, i64, vp]),
    "mms2ut_set_f32": (i32, [vp, i32, vp, vp]),
    "mms2ut_splitk_reduce": (i32, [vp, i32, i64, i32, i32, vp, i64, i32, f32, vp]),
    "mms2ut_splitk_reduce_bias": (i32, [vp, i32, i64, i32, i32, vp, i64, vp, vp, vp]),
    "mms2ut_transpose_batch": (i32, [vp, vp, vp, i32, i32, vp]),
    "mms2ut_layernorm_fwd": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, f32, vp]),
    "mms2ut_layernorm_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, f32, u64, u64, vp]),
    "mms2ut_layernorm_bwd_parts": (i32, [i64]),
    "mms2ut_layernorm_bwd_nparts": (i32, [i64, i32]),
    "mms2ut_layernorm_fwd_ex": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, f32, i64, i64, f32, u64, u64, vp]),
    "mms2ut_layernorm_bwd_ex": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, f32, u64, u64, i64, i64,
                                      f32, u64, u64, vp]),
    "mms2ut_colsum_parts": (i32, [vp, i32, i32, vp, i32, vp]),
    "mms2ut_colsum_f16": (i32, [vp, i64, i32, i64, vp, i32, vp]),
    "mms2ut_colsum_nparts": (i32, [i64]),
    "mms2ut_attn_softmax_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i64, vp, vp, i64, i32, i32,
                                      f32, u64, u64, vp]),
    "mms2ut_attn_softmax_bwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i64, vp, i32, i32, f32, u64,
                                      u64, vp]),
    "mms2ut_attn_softmax_fwd_aug": (i32, [vp, vp, vp, i32, i32, i32, i64, vp, i64, i32, f32, u64, u64,
                                          vp, i64, f32, i32, vp, i64, i32, vp]),
    "mms2ut_attn_softmax_bwd_aug": (i32, [vp, vp, vp, i32, i32, i32, i64, f32, u64, u64, vp, i64, f32, i32,
                                          vp, i64, i32, vp]),
    "mms2ut_fusion_pack_kv": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "mms2ut_fusion_unpack_kv": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "mms2ut_mha_varlen_fwd": (i32, [vp, vp]),   # ATTN_ARGS.pack(...) bytes
    "mms2ut_mha_varlen_bwd": (i32, [vp, vp, i64, i64, vp, vp, i64, i64, vp, i64, i64,
                                    vp, i64, i64, vp]),
    "mms2ut_mha_varlen_fwd_plan": (i32, [vp, vp]),
    "mms2ut_mha_varlen_bwd_plan": (i32, [vp, vp, i64, i64, vp, vp, i64, i64, vp, i64, i64,
                                         vp, i64, i64, vp]),
    "mms2ut_dropout_fwd": (i32, [vp, vp, i64, f32, u64, u64, vp]),
    "mms2ut_dropout_mask": (i32, [vp, i64, f32, u64, u64, vp]),
    "mms2ut_encoder_embed_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, f32, u64, u64, vp]),
    "mms2ut_scale_dropout_bwd": (i32, [vp, vp, i64, f32, f32, u64, u64, vp]),
    "mms2ut_token_embed_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, u64, u64, vp]),
    "mms2ut_token_embed_bwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, u64, u64, vp]),
    "mms2ut_add_f32_to_f16": (i32, [vp, vp, vp, i64, vp]),
    "mms2ut_add_f16": (i32, [vp, vp, vp, i64, vp]),
    "mms2ut_glu_fwd": (i32, [vp, vp, i64, i32, vp]),
    "mms2ut_glu_bwd": (i32, [vp, vp, vp, i64, i32, vp]),
    "mms2ut_im2col": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "mms2ut_im2col_ld": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "mms2ut_col2im": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "mms2ut_gate_bwd": (i32, [vp, vp, vp, vp, vp, i64, i32, vp]),
    "mms2ut_copy2d_pad": (i32, [vp, i64, vp, i64, i64, i32, i32, vp]),
    "mms2ut_copy2d": (i32, [vp, i64, vp, i64, i64, i32, vp]),
    "mms2ut_ls_xent_fwd": (i32, [vp, i64, vp, i64, i32, f32, i32, vp, vp, vp, vp]),
    "mms2ut_ls_xent_fwd_log": (i32, [vp, i64, vp, i64, i32, f32, i32, vp, vp, vp, vp, vp]),
    "mms2ut_ls_xent_eval": (i32, [vp, i64, vp, i64, i32, f32, i32, vp, vp, vp]),
    "mms2ut_ls_xent_bwd": (i32, [vp, i64, vp, i64, i32, f32, i32, vp, vp, vp, vp]),
    "mms2ut_ls_xent_rdrop_fwd": (i32, [vp, i64, vp, i64, i32, f32, i32, f32, vp, vp, vp, vp, vp, vp]),
    "mms2ut_ls_xent_rdrop_bwd": (i32, [vp, i64, vp, i64, i32, f32, i32, f32, vp, vp, vp, vp]),
    "mms2ut_grad_sqnorm": (i32, [vp, i64, vp, i32, vp]),
    "mms2ut_grad_norm_finalize": (i32, [vp, i32, vp, vp, vp]),
    "mms2ut_stream_wait": (i32, [vp, vp]),
    "mms2ut_bind_step_seed": (i32, [vp]),
    "mms2ut_step_seed_advance": (i32, [vp, u64, vp]),
    "mms2ut_optim_prepare": (i32, [vp, f32, f32, f32, f32, f32, f32, f32, f32, vp]),
    "mms2ut_adam_fp16_master": (i32, [vp, vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, vp]),
    "mms2ut_fbank_frames": (i32, [vp, i32, vp, vp]),
    "mms2ut_fbank_f32": (i32, [vp, vp, vp, i32, i32, vp, vp, i32, vp, vp]),
    "mms2ut_fbank_cmvn_collate": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "mms2ut_specaugment_f16": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, i32, f32, vp]),
    "mms2ut_noise_mix_f32": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, vp, vp]),
    "mms2ut_resample_plan": (i32, [i32, i32, i32, C.POINTER(C.c_int)]),
    "mms2ut_resample_f32": (i32, [vp, vp, vp, i32, i64, vp, i32, i32, i32, i32, vp, vp, vp]),
    "mms2ut_conv1d_tm_packed_halves": (i32, [i32, i32, i32, C.POINTER(C.c_int64)]),
    "mms2ut_conv1d_tm": (i32, [vp, vp]),   # CONV1D_TM_ARGS.pack(...) bytes
    "mms2ut_conv_transpose1d_tm": (i32, [vp, i64, i32, i32, vp, vp, vp, i64, i32, i32, i32, i32, i32, f32, vp]),
    "mms2ut_conv_post_tanh": (i32, [vp, i64, i32, i32, vp, f32, i32, i32, f32, vp, vp]),
    "mms2ut_embed_repeat": (i32, [vp, i32, i32, vp, i32, vp, i64, vp, vp]),
    "mms2ut_var_pred_layer_f32": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, f32, vp, vp, f32,
                                        vp, vp, vp]),
    "mms2ut_hifigan_sizes": (i32, [vp, i64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mms2ut_hifigan_fwd": (i32, [vp, vp, i32, vp, i64, vp, vp, C.POINTER(C.c_int), vp]),
    "mms2ut_wave_stats": (i32, [vp, i64, f32, vp, vp, vp]),
    "mms2ut_asr_conv0": (i32, [vp, i64, vp, vp, vp, vp, vp, f32, i32, i32, i32, vp, i64, vp]),
    "mms2ut_asr_conv": (i32, [vp, vp]),   # ASR_CONV_ARGS.pack(...) bytes
    "mms2ut_asr_ln_gelu": (i32, [vp, i64, i32, i32, vp, vp, f32, vp]),
    "mms2ut_ctc_greedy": (i32, [vp, i64, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    "mms2ut_hubert_conv0": (i32, [vp, i64, vp, vp, vp, vp, vp, f32, i32, i32, i32, vp, vp, vp, i64, vp]),
    "mms2ut_kmeans_chunks": (i32, [i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mms2ut_kmeans_assign": (i32, [vp, i64, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp]),
    "mms2ut_kmeans_fold": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "mms2ut_kmeans_topk": (i32, [vp, i64, i32, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "mms2ut_kmeans_topk_fold": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp]),
    "mms2ut_units_beam_ws": (i32, [i32, i32, i32, C.POINTER(i64)]),
    "mms2ut_units_beam": (i32, [vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
    "mms2ut_kmeans_row_norms": (i32, [vp, i64, i64, i32, vp, vp]),
    "mms2ut_kmeans_gather": (i32, [vp, i64, i64, vp, vp, i32, i32, vp, i32, vp, vp, vp]),
    "mms2ut_kmeans_train_fold": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, C.c_double, i32, vp]),
    "mms2ut_kmeans_accumulate": (i32, [vp, i64, vp, i32, i32, i32, vp, vp, vp, vp]),
    "mms2ut_kmeans_update": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
    "mms2ut_kmeans_pp": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "mms2ut_kmeans_step": (i32, [vp, vp, vp]),
    "mms2ut_vision_patches": (i32, [vp, i64, vp, i32, vp, i64, vp, vp, i32, i32, i32, vp]),
    "mms2ut_nonfinite_rows_f16": (i32, [vp, i64, i32, i64, vp, vp]),
    "mms2ut_rollout_probs_f16": (i32, [vp, vp, i64, i64, i32, i32, i32, i32, f32, i32, vp, i64, vp]),
    "mms2ut_rollout_discard_f32": (i32, [vp, i32, i64, i64, vp]),
    "mms2ut_rollout_chain_f32": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "mms2ut_ngram_stats": (i32, [vp, i64, vp, vp, i64, vp, i32, i32, i32, i32, vp, vp]),
    "mms2ut_edit_distance": (i32, [vp, i64, vp, vp, i64, vp, i32, i32, vp, vp, vp]),
    "mms2ut_layer_arena": (i32, [vp, vp, vp]),
    "mms2ut_layer_scratch": (i32, [vp, f32, vp, vp]),
    "mms2ut_layer_ws": (i32, [vp, vp, vp]),
    "mms2ut_layer_fwd": (i32, [vp, vp, i64, vp]),
    "mms2ut_layer_bwd": (i32, [vp, vp, vp, vp]),
    "mms2ut_gated_fusion_set_route": (i32, [i32]),
    "mms2ut_gated_fusion_route": (i32, [vp]),
    "mms2ut_gated_fusion_arena": (i32, [vp, vp, vp]),
    "mms2ut_gated_fusion_scratch": (i32, [vp, i32, vp, vp]),
    "mms2ut_gated_fusion_ws": (i32, [vp, vp, vp]),
    "mms2ut_gated_fusion_fwd": (i32, [vp, vp, i64, vp]),
    "mms2ut_gated_fusion_bwd": (i32, [vp, vp, i32, vp, vp, i64, vp, i64, i32, vp, vp]),
    "mms2ut_workspace_size": (i32, [i32, vp, vp]),
    "mms2ut_conv1d_glu_arena": (i32, [vp, vp, vp]),
    "mms2ut_conv1d_glu_scratch": (i32, [vp, vp, vp]),
    "mms2ut_conv1d_glu_ws": (i32, [vp, vp, vp]),
    "mms2ut_conv1d_glu_fwd": (i32, [vp, vp, i64, vp]),
    "mms2ut_conv1d_glu_bwd": (i32, [vp, vp, vp, vp, i64, vp, i64, i32, vp, vp]),
    "mms2ut_log_softmax_step": (i32, [vp, i64, i64, i32, i32, i32, i32, vp, vp]),
    "mms2ut_log_softmax_step_ext": (i32, [vp, i64, i64, i32, i32, i32, i32, i32, f32, f32, vp, vp]),
    "mms2ut_ngram_block": (i32, [vp, i64, i64, i32, i32, vp, i32, vp]),
    "mms2ut_sample_step": (i32, [vp, vp, i64, vp, i32, i32, i32, i32, i32, u64, i32, f32, vp, vp, vp, vp, vp, vp]),
    "mms2ut_kv_cache_gather": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "mms2ut_decode_self_attn": (i32, [vp, i64, vp, vp, i32, i32, i32, i32, vp, vp, i64, i64, vp, i64, f32, vp]),
    "mms2ut_decode_embed": (i32, [vp, vp, vp, vp, i32, vp, i32, i32, f32, vp]),
    "mms2ut_splitk_epilogue_f16": (i32, [vp, i32, i64, i32, i32, vp, vp, i64, i32, vp, i64, vp]),
    "mms2ut_beam_topk": (i32, [vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "mms2ut_beam_eos_scan": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "mms2ut_beam_advance": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp]),
    "mms2ut_splitk_epilogue_ln_f16": (i32, [vp, i32, i64, i32, i32, vp, vp, i64, vp, i64, vp, vp, f32, vp, i64,
                                            vp]),
}

_lib = None


class HipError(RuntimeError):
    pass


def load():
    """Load the HIP library (raises if it was not built — there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipError(f"libmms2ut_hip.so not found at {LIB_PATH}; run "
                       f"`python multimodal-s2ut_amd/build.py` (hipcc, gfx950)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def call(name, *args):
    rc = getattr(_lib or load(), name)(*args)
    if rc != 0:
        raise HipError(f"{name} failed ({rc}): {_lib.mms2ut_last_error().decode()}")
    return rc
