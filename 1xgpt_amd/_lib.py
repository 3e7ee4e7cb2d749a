"""ctypes binding of libgenie_hip.so (C ABI: include/genie_hip.h).

There is NO CPU fallback: if the library is missing or a call fails, this raises.  The oracle under
oracle/ is test infrastructure and is never imported from here.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# GENIE_HIP_LIBRARY: an explicit path to another build of the same ABI (the -DGENIE_STUDY library of 1xgpt_amd/build.py, an A/B
# variant under 1xgpt_amd/build/ab/) for tools/; unset = the shipping library beside this file
LIB_PATH = os.environ.get("GENIE_HIP_LIBRARY") or os.path.join(HERE, "libgenie_hip.so")

PREC_EXACT, PREC_BF16, PREC_F16X3 = 0, 1, 2
LAYOUT_TOKEN_MAJOR, LAYOUT_BCTHW = 0, 1
UNMASK_RANDOM, UNMASK_GREEDY, UNMASK_CONFIDENCE = 0, 1, 2
SPATIAL_BWD_AUTO, SPATIAL_BWD_FUSED, SPATIAL_BWD_MATERIALISED, SPATIAL_BWD_BF16 = 0, 1, 2, 3
KC_GEMM, KC_ATTN_SPATIAL, KC_ATTN_TEMPORAL, KC_LAYERNORM, KC_OTHER, KC_FUSED = range(6)
E_ARG, E_SHAPE, E_UNSUPPORTED, E_LAUNCH, E_ASSERT = -1, -2, -3, -4, -5

c_f32p = C.c_void_p  # device pointers travel as plain integers
c_ptr = C.c_void_p


class GenieCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "num_layers", "num_heads", "head_dim", "d_model", "T", "S", "hidden", "factored_vocab", "num_factored",
        "image_vocab_size", "qk_norm", "use_mup", "qkv_bias", "proj_bias", "mlp_bias")] + [
        ("attn_scale", C.c_float), ("readout_mult", C.c_float), ("precision", C.c_int32)]


class AttnWeights(C.Structure):
    _fields_ = [(n, c_ptr) for n in ("qkv_w", "qkv_b", "proj_w", "proj_b", "norm_w", "norm_b", "qkv_w16", "proj_w16",
                                     "fused_w16")] + [("w16_wide", C.c_int32), ("frame_w16", c_ptr)]


class LayerWeights(C.Structure):
    _fields_ = [("norm1_w", c_ptr), ("norm1_b", c_ptr), ("spatial", AttnWeights), ("temporal", AttnWeights),
                ("norm2_w", c_ptr), ("norm2_b", c_ptr), ("fc1_w", c_ptr), ("fc1_b", c_ptr), ("fc2_w", c_ptr),
                ("fc2_b", c_ptr), ("fc1_w16", c_ptr), ("fc2_w16", c_ptr), ("mlp_fused_w16", c_ptr), ("w16_wide", C.c_int32),
                ("mlp_frame_w16", c_ptr)]


class Weights(C.Structure):
    _fields_ = [("pos_embed", c_ptr), ("mask_embed", c_ptr), ("embed", c_ptr * 4), ("out_w", c_ptr),
                ("out_b", c_ptr), ("out_w16", c_ptr), ("layers_host", C.POINTER(LayerWeights)), ("out_w16_wide", C.c_int32),
                ("out_frame_w16", c_ptr)]

class FrameCond(C.Structure):
    """genie_frame_cond: per-frame action conditioning (table (n_actions, d) f32 and ids (B, T) int64, device pointers)."""
    _fields_ = [("table", c_ptr), ("ids", c_ptr), ("n_actions", C.c_int32)]


class Sampling(C.Structure):
    """genie_sampling: logit temperature, top-k, top-p, choice temperature of the "confidence" unmasking (1xgpt_amd/sampling.py)."""
    _fields_ = [("logit_temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("choice_temperature", C.c_float)]


class Guidance(C.Structure):
    """genie_guidance: classifier-free guidance scale w and the action-table row of the null action (1xgpt_amd/sampling.py)."""
    _fields_ = [("scale", C.c_float), ("null_action", C.c_int32)]


class Known(C.Structure):
    """genie_known: the known tokens of the frames a generate call decodes (device pointer, clip stride in elements); a value outside
    [0, image_vocab_size) marks a token to generate (1xgpt_amd/generate.py: known_tokens)."""
    _fields_ = [("ids", c_ptr), ("clip_stride", C.c_int64)]


class ActionProj(C.Structure):
    """genie_action_proj: the projection of continuous per-frame action vectors (weight (d, A), bias, input mean and 1/std; device pointers)."""
    _fields_ = [("weight", c_ptr), ("bias", c_ptr), ("mean", c_ptr), ("inv_std", c_ptr), ("action_dim", C.c_int32)]


class Dropout(C.Structure):
    """genie_dropout: MLP dropout of one training micro-batch (drop probability, micro-batch counter, seed; 1xgpt_amd/train.py)."""
    _fields_ = [("p", C.c_float), ("call", C.c_uint32), ("seed", C.c_uint64)]


class Objective(C.Structure):
    """genie_objective: label smoothing, z-loss and per-frame loss weights of the training step (1xgpt_amd/train.py); n_frames 0 = all
    frames weigh 1, else T."""
    _fields_ = [("label_smoothing", C.c_float), ("z_loss", C.c_float), ("n_frames", C.c_int32), ("reserved", C.c_int32),
                ("frame_weight", C.c_float * 64)]


class Distill(C.Structure):
    """genie_distill: mix alpha, temperature and the teacher's logits (device pointer, read only) of one training micro-batch
    (1xgpt_amd/train.py); alpha 0 = no distillation."""
    _fields_ = [("alpha", C.c_float), ("temperature", C.c_float), ("teacher_logits", c_ptr)]


class LoraItem(C.Structure):
    """genie_lora_item: one adapted Linear of a genie_lora_merge / genie_lora_project call (device pointers; 1xgpt_amd/lora.py)."""
    _fields_ = [(n, c_ptr) for n in ("w", "w0", "a", "b", "dw", "da", "db")] + [(n, C.c_int32) for n in ("out", "in_", "rank")] + [
        ("scale", C.c_float)]


LORA_MAX_ITEMS, LORA_MAX_RANK = 8, 64   # GENIE_LORA_MAX_ITEMS, GENIE_LORA_MAX_RANK


class MuonItem(C.Structure):
    """genie_muon_item: one target matrix of a genie_muon_step call (device pointers; 1xgpt_amd/muon.py)."""
    _fields_ = [(n, c_ptr) for n in ("param", "grad", "momentum", "ema")] + [("rows", C.c_int32), ("cols", C.c_int32), ("lr", C.c_float),
                                                                             ("weight_decay", C.c_float)]


class MuonSettings(C.Structure):
    """genie_muon_settings."""
    _fields_ = [(n, C.c_float) for n in ("momentum", "a", "b", "c", "eps", "grad_mult", "max_grad_norm", "ema_one_minus_decay")] + [
        (n, C.c_int32) for n in ("nesterov", "ns_steps", "adjust", "reserved")] + [("grad_sumsq", c_ptr)]


MUON_MAX_ITEMS = 64   # GENIE_MUON_MAX_ITEMS
MUON_ADJUST = {"original": 0, "match_rms_adamw": 1}   # GENIE_MUON_ADJUST_*
ACTION_MAX_DIM = 256   # GENIE_ACTION_MAX_DIM
WIDE_QKV, WIDE_PROJ, WIDE_FC1, WIDE_FC2 = 1, 2, 1, 2          # bits of the w16_wide fields (genie_hip.h)
FUSED_QKV_STREAM = 4                                        # spatial attention: fused_w16 = [proj stream | qkv stream]
TEMPORAL_QKV_F16X3_ELEMS = 393216   # f16 values of the f16x3 temporal qkv stream (csrc/kernels_fused_f16x3.hip)
TEMPORAL_FUSED_ELEMS, MLP_FUSED_ELEMS, SPATIAL_PROJ_FUSED_ELEMS, SPATIAL_QKV_FUSED_ELEMS = 262144, 524288, 65536, 196608        # bf16 values of the fused kernels' weight streams
ABI_VERSION = 3


# name -> (restype, argtypes); must list every symbol include/genie_hip.h declares
SIGNATURES = {
    "genie_version": (C.c_int, []),
    "genie_abi_layout": (C.c_int, [C.POINTER(C.c_size_t), C.c_int]),
    "genie_sampling_layout": (C.c_int, [C.POINTER(C.c_size_t), C.c_int]),
    "genie_guidance_layout": (C.c_int, [C.POINTER(C.c_size_t), C.c_int]),
    "genie_action_proj_layout": (C.c_int, [C.POINTER(C.c_size_t), C.c_int]),
    "genie_action_rows": (C.c_int, [C.POINTER(ActionProj), c_ptr, c_ptr, C.c_int64, C.c_int, c_ptr]),
    "genie_action_rows_backward": (C.c_int, [C.POINTER(ActionProj), c_ptr, c_ptr, C.c_int64, C.c_int, c_ptr, c_ptr, C.c_int, c_ptr]),
    "genie_last_error": (C.c_char_p, []),
    "genie_check_config": (C.c_int, [C.POINTER(GenieCfg)]),
    "genie_workspace_bytes": (C.c_size_t, [C.POINTER(GenieCfg), C.c_int]),
    "genie_pack_bf16": (C.c_int, [c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_pack_split_f16": (C.c_int, [c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_embed": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, c_ptr, c_ptr]),
    "genie_layer_norm": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_float, c_ptr]),
    "genie_linear": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_linear_lowp": (C.c_int, [C.c_int, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    c_ptr]),
    "genie_spatial_attention": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(AttnWeights), c_ptr, c_ptr, C.c_int, c_ptr]),
    "genie_temporal_attention": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(AttnWeights), c_ptr, c_ptr, C.c_int, c_ptr]),
    "genie_attention_core": (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, c_ptr,
                                       c_ptr, c_ptr]),
    "genie_st_block_forward": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(LayerWeights), c_ptr, C.c_int, c_ptr,
                                         C.c_size_t, c_ptr]),
    "genie_decoder_forward": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, c_ptr, C.c_size_t,
                                        c_ptr]),
    "genie_readout_logits": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, C.c_int, C.c_int,
                                       C.c_int, c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_compute_logits": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, C.c_int, C.c_int,
                                       C.c_int, c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_prefix_cache_bytes": (C.c_size_t, [C.POINTER(GenieCfg), C.c_int]),
    "genie_clean_pass": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, C.c_int, C.c_int, c_ptr,
                                   C.c_size_t, c_ptr, C.c_size_t, c_ptr]),
    "genie_masked_frames_logits": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, C.c_int, C.c_int, c_ptr,
                                             C.c_size_t, c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_frame_pass": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, C.c_int, c_ptr, C.c_size_t,
                                   c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_frames_pass": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, C.c_int, C.c_int, c_ptr, C.c_size_t,
                                    c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_generate_workspace_bytes": (C.c_size_t, [C.POINTER(GenieCfg), C.c_int, C.c_int]),
    "genie_generate_guided_workspace_bytes": (C.c_size_t, [C.POINTER(GenieCfg), C.c_int, C.c_int]),
    "genie_guide_logits": (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_size_t, C.c_float, c_ptr]),
    "genie_generate_cached": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                        C.c_int, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, c_ptr, c_ptr, C.c_size_t, c_ptr, C.c_size_t, c_ptr]),
    "genie_pack_frame_w16": (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, c_ptr]),
    "genie_frame_linear": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_metric_hits": (C.c_int, [c_ptr, C.c_int64, c_ptr, C.c_int64, C.c_int, C.c_int64, c_ptr, C.c_double, C.c_double,
                                    C.c_double, c_ptr, c_ptr]),
    "genie_factored_ce": (C.c_int, [C.POINTER(GenieCfg), c_ptr, C.c_int, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int,
                                    c_ptr, c_ptr]),
    "genie_readout_ce": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, c_ptr, c_ptr, C.c_int, C.c_int,
                                   C.c_int, c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_train_activation_bytes": (C.c_size_t, [C.POINTER(GenieCfg), C.c_int]),
    "genie_train_workspace_bytes": (C.c_size_t, [C.POINTER(GenieCfg), C.c_int]),
    "genie_train_forward": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, c_ptr, C.c_int, c_ptr, C.c_size_t,
                                      c_ptr, c_ptr]),
    "genie_train_pack_weights": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), C.POINTER(Weights),
                                           C.POINTER(Weights), c_ptr]),
    "genie_train_backward_head": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), C.POINTER(Weights),
                                            C.POINTER(Weights), C.c_int, c_ptr, c_ptr, C.c_size_t, C.c_int, c_ptr]),
    "genie_train_backward_layer": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), C.POINTER(Weights),
                                             C.POINTER(Weights), C.c_int, C.c_int, c_ptr, c_ptr, C.c_size_t, C.c_int,
                                             c_ptr]),
    "genie_train_backward_embed": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, c_ptr, C.c_size_t,
                                             C.c_int, c_ptr]),
    "genie_train_backward_embed_cond": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, c_ptr, C.c_size_t,
                                                  C.c_int, c_ptr, c_ptr, C.POINTER(FrameCond)]),
    "genie_temporal_attention_backward": (C.c_int, [c_ptr, c_ptr, C.c_int64, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, C.c_float, c_ptr]),
    "genie_spatial_attention_backward_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "genie_spatial_attention_backward": (C.c_int, [c_ptr, c_ptr, C.c_int64, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_int, C.c_float, C.c_int, c_ptr, C.c_size_t, c_ptr]),
    "genie_qk_norm_forward": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int64, C.c_int, C.c_int, c_ptr]),
    "genie_qk_norm_backward_scratch_bytes": (C.c_size_t, [C.c_int]),
    "genie_qk_norm_backward": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int64, C.c_int, C.c_int, C.c_int, c_ptr,
                                         C.c_size_t, c_ptr]),
    "genie_sumsq": (C.c_int, [c_ptr, C.c_size_t, c_ptr, c_ptr, c_ptr]),
    "genie_adamw_step": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_int, C.c_float, c_ptr, C.c_float, c_ptr]),
    "genie_sample": (C.c_int, [C.POINTER(GenieCfg), c_ptr, C.c_int, C.c_int, C.c_float, c_ptr, c_ptr, c_ptr, c_ptr]),
    "genie_mask_step": (C.c_int, [c_ptr, C.c_int, C.c_int, C.c_int64, c_ptr, c_ptr, c_ptr, C.c_int64, C.c_int,
                                  C.c_int, c_ptr]),
    "genie_maskgit_generate": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr, C.c_int, C.c_int, C.c_int,
                                         C.c_float, C.c_int, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, c_ptr, c_ptr,
                                         C.c_size_t, c_ptr]),
    "genie_profile_enable": (C.c_int, [C.c_int]),
    "genie_profile_reset": (C.c_int, []),
    "genie_profile_read": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "genie_profile_kernels": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "genie_study_build": (C.c_int, []),
    "genie_pack_temporal_fused_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr]),
    "genie_pack_temporal_qkv_f16x3": (C.c_int, [c_ptr, c_ptr, c_ptr]),
    "genie_temporal_prefix_fused_bf16": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(AttnWeights), c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_temporal_qkv_attn_f16x3": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(AttnWeights), c_ptr, c_ptr, C.c_int64, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_pack_mlp_fused_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr]),
    "genie_pack_spatial_proj_fused_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr]),
    "genie_pack_spatial_qkv_fused_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr]),
    "genie_mlp_fused_qkv_bf16": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(LayerWeights), C.POINTER(LayerWeights), c_ptr, c_ptr, C.c_int64, c_ptr]),
    "genie_spatial_attn_proj_fused_bf16": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(AttnWeights), c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    "genie_temporal_fused_bf16": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(AttnWeights), c_ptr, c_ptr, C.c_int, c_ptr]),
    "genie_mlp_fused_bf16": (C.c_int, [C.POINTER(GenieCfg), C.POINTER(LayerWeights), c_ptr, c_ptr, C.c_int64, c_ptr, c_ptr, c_ptr]),
    "genie_bits_from_tokens": (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_rescale_u8_bf16": (C.c_int, [c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_rescale_u8_f32": (C.c_int, [c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "genie_pack_conv_weight": (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_conv3x3_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, c_ptr]),
    "genie_conv3x3_s2_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        c_ptr]),
    "genie_frames_to_nhwc_bf16": (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_tokens_from_code_nhwc_bf16": (C.c_int, [c_ptr, c_ptr, C.c_int64, C.c_int, C.c_int, c_ptr]),
    "genie_conv1x1_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_conv_direct_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         c_ptr]),
    "genie_conv_gn_part_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "genie_conv3x3_gn_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, c_ptr, C.c_int, c_ptr]),
    "genie_group_norm_swish_fused_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, c_ptr]),
    "genie_group_norm_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "genie_group_norm_swish_bf16": (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_float, C.c_int, c_ptr]),
    "genie_bits_from_tokens_nhwc_bf16": (C.c_int, [c_ptr, c_ptr, C.c_int64, C.c_int, C.c_int, c_ptr]),
    "genie_rescale_u8_nhwc_bf16": (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    "genie_tokens_from_bits": (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr]),
}

# the *_cond variants: the plain entry point's arguments + a trailing genie_frame_cond* (NULL = unconditioned)
for _n in ("genie_embed", "genie_compute_logits", "genie_maskgit_generate", "genie_clean_pass", "genie_masked_frames_logits",
           "genie_frame_pass", "genie_frames_pass", "genie_generate_cached", "genie_train_forward"):
    SIGNATURES[_n + "_cond"] = (SIGNATURES[_n][0], SIGNATURES[_n][1] + [C.POINTER(FrameCond)])
del _n
# the training step with activation recomputation: the arguments of the plain entry point (genie_train_forward: of its *_cond form)
# + a trailing int recompute (0 = that entry point)
for _n in ("genie_train_activation_bytes", "genie_train_workspace_bytes", "genie_train_forward_cond", "genie_train_backward_head",
           "genie_train_backward_layer"):
    SIGNATURES[_n.replace("_cond", "") + "_ex"] = (SIGNATURES[_n][0], SIGNATURES[_n][1] + [C.c_int])
del _n
# the *_ex variants: the *_cond arguments + a trailing genie_sampling* (NULL = the *_cond entry point); genie_sample_ex: genie_sample's
# arguments + sampling, keys_out, noise, anneal
for _n in ("genie_maskgit_generate", "genie_generate_cached"):
    SIGNATURES[_n + "_ex"] = (SIGNATURES[_n][0], SIGNATURES[_n + "_cond"][1] + [C.POINTER(Sampling)])
del _n
SIGNATURES["genie_sample_ex"] = (C.c_int, SIGNATURES["genie_sample"][1] + [C.POINTER(Sampling), c_ptr, c_ptr, C.c_float])
# the *_guided variants: the *_ex arguments + a trailing genie_guidance* (NULL = the *_ex entry point); genie_sample_guided: genie_sample_ex
# with a second logits pointer (the null logits) after the first and a trailing scale
for _n in ("genie_maskgit_generate", "genie_generate_cached"):
    SIGNATURES[_n + "_guided"] = (SIGNATURES[_n][0], SIGNATURES[_n + "_ex"][1] + [C.POINTER(Guidance)])
del _n
SIGNATURES["genie_sample_guided"] = (C.c_int, SIGNATURES["genie_sample_ex"][1][:2] + [c_ptr] + SIGNATURES["genie_sample_ex"][1][2:]
                                     + [C.c_float])
# the rollout past the window: (cfg, B, ctx_max, guided) and (cfg, w, frames, B, P, keep, cap, f0, f1, resume, steps, temperature, unmask_mode,
# noise, uniforms, merge_commit, cache, cache_bytes, workspace, workspace_bytes, stream, cond, sampling, guidance)
SIGNATURES["genie_rollout_workspace_bytes"] = (C.c_size_t, [C.POINTER(GenieCfg), C.c_int, C.c_int, C.c_int])
SIGNATURES["genie_rollout_cached"] = (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr] + [C.c_int] * 8 + [C.c_float, C.c_int, c_ptr,
                                                c_ptr, C.c_int, c_ptr, C.c_size_t, c_ptr, C.c_size_t, c_ptr, C.POINTER(FrameCond),
                                                C.POINTER(Sampling), C.POINTER(Guidance)])

# fan-out generation: (cfg, NB, K, n_new), (cfg, B, K, P, guided) and (cfg, w, ids, B, K, P, n_new, steps, temperature, unmask_mode, noise,
# uniforms, merge_commit, gen_out, trunk, trunk_bytes, branch, branch_bytes, workspace, workspace_bytes, stream, cond, sampling, guidance);
# the decode attention alone: (cfg, aw, trunk_slice, branch_slice, out, NBK, K, P0, Tb, t, in16, stream)
SIGNATURES["genie_fanout_branch_bytes"] = (C.c_size_t, [C.POINTER(GenieCfg), C.c_int, C.c_int, C.c_int])
SIGNATURES["genie_fanout_workspace_bytes"] = (C.c_size_t, [C.POINTER(GenieCfg), C.c_int, C.c_int, C.c_int, C.c_int])
SIGNATURES["genie_generate_fanout"] = (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr] + [C.c_int] * 5 + [C.c_float, C.c_int, c_ptr,
                                                 c_ptr, C.c_int, c_ptr, c_ptr, C.c_size_t, c_ptr, C.c_size_t, c_ptr, C.c_size_t, c_ptr,
                                                 C.POINTER(FrameCond), C.POINTER(Sampling), C.POINTER(Guidance)])
SIGNATURES["genie_temporal_attention_decode_fanout"] = (C.c_int, [C.POINTER(GenieCfg), C.POINTER(AttnWeights), c_ptr, c_ptr, c_ptr] + [C.c_int] * 6
                                                        + [c_ptr])
# scoring observed futures: (cfg, logits, targets, target_clip_stride, K, N, nll, nll_stride, hits, token_nll, token_stride, stream),
# (cfg, B, K, P) and (cfg, w, ids, B, K, P, n, merge_commit, nll, hits, token_nll, trunk, trunk_bytes, branch, branch_bytes, workspace,
# workspace_bytes, stream, cond)
SIGNATURES["genie_score_logits"] = (C.c_int, [C.POINTER(GenieCfg), c_ptr, c_ptr, C.c_int64, C.c_int, C.c_int64, c_ptr, C.c_int64, c_ptr, c_ptr,
                                              C.c_int64, c_ptr])
SIGNATURES["genie_score_workspace_bytes"] = (C.c_size_t, [C.POINTER(GenieCfg), C.c_int, C.c_int, C.c_int])
SIGNATURES["genie_score_fanout"] = (C.c_int, [C.POINTER(GenieCfg), C.POINTER(Weights), c_ptr] + [C.c_int] * 5 + [c_ptr, c_ptr, c_ptr, c_ptr,
                                              C.c_size_t, c_ptr, C.c_size_t, c_ptr, C.c_size_t, c_ptr, C.POINTER(FrameCond)])

# known tokens: the start state of a frame, (known, known_clip_stride, mask_id, frame, frame_clip_stride, unmasked, B, S, copies, stream);
# genie_mask_step with a double `frac` for n and (known, known_clip_stride) behind mask_id; the four loops: the arguments of the widest
# existing variant + a trailing genie_known* (NULL = that variant)
SIGNATURES["genie_known_layout"] = (C.c_int, [C.POINTER(C.c_size_t), C.c_int])
SIGNATURES["genie_mask_fraction"] = (C.c_double, [C.c_int, C.c_int])
SIGNATURES["genie_known_begin"] = (C.c_int, [c_ptr, C.c_int64, C.c_int64, c_ptr, C.c_int64, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr])
SIGNATURES["genie_mask_step_known"] = (C.c_int, [c_ptr, C.c_double, C.c_int, C.c_int64, c_ptr, C.c_int64, c_ptr, c_ptr, c_ptr, C.c_int64, C.c_int,
                                                 C.c_int, c_ptr])
for _n, _w in (("genie_maskgit_generate", "genie_maskgit_generate_guided"), ("genie_generate_cached", "genie_generate_cached_guided"),
               ("genie_rollout_cached", "genie_rollout_cached"), ("genie_generate_fanout", "genie_generate_fanout")):
    SIGNATURES[_n + "_known"] = (C.c_int, SIGNATURES[_w][1] + [C.POINTER(Known)])
del _n, _w

# MLP dropout in the training step: the mask law alone, (dr, layer, site, n, keep, stream), and the *_ex arguments + a trailing
# genie_dropout* (NULL or p = 0: the *_ex entry point)
SIGNATURES["genie_dropout_layout"] = (C.c_int, [C.POINTER(C.c_size_t), C.c_int])
SIGNATURES["genie_dropout_mask"] = (C.c_int, [C.POINTER(Dropout), C.c_int, C.c_int, C.c_int64, c_ptr, c_ptr])
for _n in ("genie_train_forward", "genie_train_backward_layer"):
    SIGNATURES[_n + "_drop"] = (SIGNATURES[_n + "_ex"][0], SIGNATURES[_n + "_ex"][1] + [C.POINTER(Dropout)])
del _n

# the training objective: genie_train_forward_drop's arguments + a trailing genie_objective* (NULL or neutral: that entry point), and the
# loss launch alone, (logits, ids, labels, n_clips, T, S, vf, nfac, mask_id, obj, sums, stream)
SIGNATURES["genie_objective_layout"] = (C.c_int, [C.POINTER(C.c_size_t), C.c_int])
SIGNATURES["genie_train_forward_obj"] = (C.c_int, SIGNATURES["genie_train_forward_drop"][1] + [C.POINTER(Objective)])
SIGNATURES["genie_ce_objective"] = (C.c_int, [c_ptr, c_ptr, c_ptr] + [C.c_int] * 5 + [C.c_int64, C.POINTER(Objective), c_ptr, c_ptr])

# distillation: genie_train_forward_obj's arguments + a trailing genie_distill* (NULL or alpha = 0: that entry point), and the loss
# launch alone, genie_ce_objective's arguments with teacher_logits behind logits and the genie_distill* behind the objective
SIGNATURES["genie_distill_layout"] = (C.c_int, [C.POINTER(C.c_size_t), C.c_int])
SIGNATURES["genie_train_forward_distill"] = (C.c_int, SIGNATURES["genie_train_forward_obj"][1] + [C.POINTER(Distill)])
SIGNATURES["genie_ce_distill"] = (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr] + [C.c_int] * 5 + [C.c_int64, C.POINTER(Objective), C.POINTER(Distill),
                                            c_ptr, c_ptr])

# EMA of the weights: genie_adamw_step's arguments with `ema` behind exp_avg_sq and one_minus_decay in front of the stream; the EMA
# line alone, (ema, params, n, one_minus_decay, stream); the in-place exchange, (a, b, n, stream)
_a = SIGNATURES["genie_adamw_step"][1]
SIGNATURES["genie_adamw_ema_step"] = (C.c_int, _a[:4] + [c_ptr] + _a[4:-1] + [C.c_float, c_ptr])
del _a
SIGNATURES["genie_ema_update"] = (C.c_int, [c_ptr, c_ptr, C.c_size_t, C.c_float, c_ptr])
SIGNATURES["genie_swap_f32"] = (C.c_int, [c_ptr, c_ptr, C.c_size_t, c_ptr])

# frozen tensors: genie_train_pack_weights' arguments with a `select` table (NULL = every Linear) in front of the stream
_a = SIGNATURES["genie_train_pack_weights"][1]
SIGNATURES["genie_train_pack_weights_some"] = (C.c_int, _a[:-1] + [C.POINTER(Weights), c_ptr])
del _a

# LoRA adapters: (items, n, stream), (items, n) and (items, n, accumulate, scratch, scratch_bytes, stream)
SIGNATURES["genie_lora_layout"] = (C.c_int, [C.POINTER(C.c_size_t), C.c_int])
SIGNATURES["genie_lora_merge"] = (C.c_int, [C.POINTER(LoraItem), C.c_int, c_ptr])
SIGNATURES["genie_lora_project_scratch_bytes"] = (C.c_size_t, [C.POINTER(LoraItem), C.c_int])
SIGNATURES["genie_lora_project"] = (C.c_int, [C.POINTER(LoraItem), C.c_int, C.c_int, c_ptr, C.c_size_t, c_ptr])

# Muon: (items, n), (items, n, settings, workspace, workspace_bytes, stream) and the unit entry point of the iteration alone
SIGNATURES["genie_muon_layout"] = (C.c_int, [C.POINTER(C.c_size_t), C.c_int])
SIGNATURES["genie_muon_workspace_bytes"] = (C.c_size_t, [C.POINTER(MuonItem), C.c_int])
SIGNATURES["genie_muon_step"] = (C.c_int, [C.POINTER(MuonItem), C.c_int, C.POINTER(MuonSettings), c_ptr, C.c_size_t, c_ptr])
SIGNATURES["genie_newton_schulz"] = (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                               c_ptr, C.c_size_t, c_ptr])

# image-space metrics: (n, C, H, W) and (a, b, n, C, H, W, out, workspace, workspace_bytes, stream)
SIGNATURES["genie_frame_metrics_workspace_bytes"] = (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int])
SIGNATURES["genie_frame_metrics"] = (C.c_int, [c_ptr, c_ptr, C.c_int64, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr, C.c_size_t, c_ptr])

_lib = None


class GenieHipError(RuntimeError):
    def __init__(self, code, where, msg):
        super().__init__(f"{where}: libgenie_hip error {code}: {msg}")
        self.code = code


def load():
    """Load (once) and type the shared library.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python 1xgpt_amd/build.py` "
                "(or __graft_entry__.build()).  There is no CPU fallback for the HIP path.")
        # torch FIRST: it ships its own HIP runtime (torch/lib/libamdhip64.so, same soname as the /opt/rocm one this library links), and the
        # process must end up with ONE runtime -- torch's, whose streams and device pointers the library is handed.  Loaded the other way
        # round (this library before torch, e.g. __graft_entry__.build() followed by smoke() in one process) the library's launches fail with
        # "no ROCm-capable device is detected" on the GPU box.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        other = bool(os.environ.get("GENIE_HIP_LIBRARY"))
        missing = []
        for name, (res, args) in SIGNATURES.items():
            if other and not hasattr(lib, name):   # an A/B against an older build of this ABI: entry points added since stay unbound
                missing.append(name)
                continue
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        if lib.genie_version() != ABI_VERSION:
            raise RuntimeError(f"libgenie_hip ABI version {lib.genie_version()} != {ABI_VERSION}")
        lay = (C.c_size_t * 6)()
        mine = [C.sizeof(ActionProj)] + [getattr(ActionProj, n).offset for n, _ in ActionProj._fields_]
        if lib.genie_action_proj_layout(lay, 6) != 6 or list(lay) != mine:
            raise RuntimeError(f"genie_action_proj layout {list(lay)} != the ctypes declaration {mine}")
        mine = [C.sizeof(Sampling)] + [getattr(Sampling, n).offset for n, _ in Sampling._fields_]
        if lib.genie_sampling_layout(lay, 5) != 5 or list(lay)[:5] != mine:
            raise RuntimeError(f"genie_sampling layout {list(lay)[:5]} != the ctypes declaration {mine}")
        mine = [C.sizeof(Guidance)] + [getattr(Guidance, n).offset for n, _ in Guidance._fields_]
        if lib.genie_guidance_layout(lay, 3) != 3 or list(lay)[:3] != mine:
            raise RuntimeError(f"genie_guidance layout {list(lay)[:3]} != the ctypes declaration {mine}")
        mine = [C.sizeof(Known)] + [getattr(Known, n).offset for n, _ in Known._fields_]
        if "genie_known_layout" not in missing and (lib.genie_known_layout(lay, 3) != 3 or list(lay)[:3] != mine):
            raise RuntimeError(f"genie_known layout {list(lay)[:3]} != the ctypes declaration {mine}")
        mine = [C.sizeof(Dropout)] + [getattr(Dropout, n).offset for n, _ in Dropout._fields_]
        if "genie_dropout_layout" not in missing and (lib.genie_dropout_layout(lay, 4) != 4 or list(lay)[:4] != mine):
            raise RuntimeError(f"genie_dropout layout {list(lay)[:4]} != the ctypes declaration {mine}")
        mine = [C.sizeof(Objective)] + [getattr(Objective, n).offset for n, _ in Objective._fields_]
        if "genie_objective_layout" not in missing and (lib.genie_objective_layout(lay, 6) != 6 or list(lay) != mine):
            raise RuntimeError(f"genie_objective layout {list(lay)} != the ctypes declaration {mine}")
        mine = [C.sizeof(Distill)] + [getattr(Distill, n).offset for n, _ in Distill._fields_]
        if "genie_distill_layout" not in missing and (lib.genie_distill_layout(lay, 4) != 4 or list(lay)[:4] != mine):
            raise RuntimeError(f"genie_distill layout {list(lay)[:4]} != the ctypes declaration {mine}")
        lay = (C.c_size_t * 12)()
        mine = [C.sizeof(LoraItem)] + [getattr(LoraItem, n).offset for n, _ in LoraItem._fields_]
        if "genie_lora_layout" not in missing and (lib.genie_lora_layout(lay, 12) != 12 or list(lay) != mine):
            raise RuntimeError(f"genie_lora_item layout {list(lay)} != the ctypes declaration {mine}")
        lay = (C.c_size_t * 23)()
        mine = [v for T in (MuonItem, MuonSettings) for v in [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_]]
        if "genie_muon_layout" not in missing and (lib.genie_muon_layout(lay, 23) != 23 or list(lay) != mine):
            raise RuntimeError(f"genie_muon_item / genie_muon_settings layout {list(lay)} != the ctypes declaration {mine}")
        if os.environ.get("GENIE_HIP_LIBRARY") or lib.genie_study_build():
            import sys
            print(f"1xgpt_amd: using {LIB_PATH} (study build: {bool(lib.genie_study_build())}) -- not the shipping library"
                  + (f"; it lacks {', '.join(missing)}" if missing else ""), file=sys.stderr)
        _lib = lib
    return _lib


def check(rc, where):
    if rc != 0:
        msg = load().genie_last_error().decode(errors="replace")
        if rc == E_ASSERT:
            raise AssertionError(msg)
        if rc == E_UNSUPPORTED and "unmask_mode" in msg:
            raise NotImplementedError(msg)
        raise GenieHipError(rc, where, msg)


def call_cond(lib, name, cond, *args):
    """lib.<name>(*args) when `cond` is None (the unconditioned entry point, unchanged), else lib.<name>_cond(*args, cond)."""
    if cond is None:
        return getattr(lib, name)(*args)
    return getattr(lib, name + "_cond")(*args, cond)


def call_recompute(lib, name, recompute, *args, cond=False):
    """lib.<name>(*args) when `recompute` is 0 (the saving training step's entry point, unchanged), else lib.<name>_ex(*args, recompute).
    cond: False for an entry point without conditioning; for genie_train_forward, None or the genie_frame_cond of the call: call_cond
    when `recompute` is 0, else lib.<name>_ex(*args, cond, recompute)."""
    if cond is False:
        return getattr(lib, name + "_ex")(*args, recompute) if recompute else getattr(lib, name)(*args)
    return getattr(lib, name + "_ex")(*args, cond, recompute) if recompute else call_cond(lib, name, cond, *args)


def call_drop(lib, name, recompute, drop, *args, cond=False):
    """call_recompute when `drop` is None (the entry points of before, unchanged), else lib.<name>_drop(*args, [cond,] recompute, drop)."""
    if drop is None:
        return call_recompute(lib, name, recompute, *args, cond=cond)
    if cond is False:
        return getattr(lib, name + "_drop")(*args, recompute, drop)
    return getattr(lib, name + "_drop")(*args, cond, recompute, drop)


def call_ex(lib, name, cond, sampling, *args):
    """call_cond when `sampling` is None (the entry points of before, unchanged), else lib.<name>_ex(*args, cond, sampling)."""
    if sampling is None:
        return call_cond(lib, name, cond, *args)
    return getattr(lib, name + "_ex")(*args, cond, sampling)


def call_guided(lib, name, cond, sampling, guidance, *args):
    """call_ex when `guidance` is None (the entry points of before, unchanged), else lib.<name>_guided(*args, cond, sampling, guidance)."""
    if guidance is None:
        return call_ex(lib, name, cond, sampling, *args)
    return getattr(lib, name + "_guided")(*args, cond, sampling, guidance)


def call_known(lib, name, cond, sampling, guidance, known, *args):
    """call_guided when `known` is None (the entry points of before, unchanged), else lib.<name>_known(*args, cond, sampling, guidance,
    known).  For genie_rollout_cached and genie_generate_fanout, whose one entry point already takes all three, use call_known3."""
    if known is None:
        return call_guided(lib, name, cond, sampling, guidance, *args)
    return getattr(lib, name + "_known")(*args, cond, sampling, guidance, known)


def call_known3(lib, name, known, *args):
    """lib.<name>(*args) when `known` is None (unchanged), else lib.<name>_known(*args, known): genie_rollout_cached, genie_generate_fanout."""
    if known is None:
        return getattr(lib, name)(*args)
    return getattr(lib, name + "_known")(*args, known)


def make_known(known, frames, S):
    """The genie_known of a contiguous int64 device tensor whose trailing dimensions are (frames, S)-many elements per clip; None -> None."""
    if known is None:
        return None
    return Known(known.data_ptr(), int(frames) * int(S))


def make_cfg(config, precision=PREC_EXACT) -> GenieCfg:
    return GenieCfg(
        num_layers=config.num_layers, num_heads=config.num_heads, head_dim=config.d_model // config.num_heads,
        d_model=config.d_model, T=config.T, S=config.S, hidden=int(config.d_model * config.mlp_ratio),
        factored_vocab=config.factored_vocab_size, num_factored=config.num_factored_vocabs,
        image_vocab_size=config.image_vocab_size, qk_norm=int(config.qk_norm), use_mup=int(config.use_mup),
        qkv_bias=int(config.qkv_bias), proj_bias=int(config.proj_bias), mlp_bias=int(config.mlp_bias),
        attn_scale=config.attn_scale, readout_mult=config.readout_mult, precision=precision)
