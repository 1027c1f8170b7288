"""ctypes binding of libsdhip.so (the C ABI declared in include/sd_hip.h).

There is NO fallback: if the library is missing or a symbol is absent this module raises, and
every product path above it fails loudly.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SD_AMD_LIB", os.path.join(HERE, "lib", "libsdhip.so"))   # (SD_AMD_LIB: A/B builds of the kernels)
HEADER_PATH = os.path.normpath(os.path.join(HERE, "..", "include", "sd_hip.h"))

# the SD_ABLATE build of the same sources (build.py): timing-ablation kernels that produce WRONG results by design
# (sd_op_conv3x3_ablate's DIAG modes, SD_GEMM_TUNE) live ONLY there -- tools/, bench.py's MFMA-stream probe and one test load it
ABLATE_LIB_PATH = os.path.join(HERE, "lib", "libsdhip_ablate.so")

_lib: Optional[C.CDLL] = None
_ablate: Optional[C.CDLL] = None


class SdUnetConfig(C.Structure):
    """The fields of ``sd_unet_config`` up to the IP-Adapter's: only the PREFIX of what the library reads.  Never passed to an
    entry point (their argument type is ``SdUnetConfigFull``, so ctypes refuses this one); kept as the base of the full struct."""
    _fields_ = [
        ("sample_size", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int),
        ("num_levels", C.c_int), ("block_out_channels", C.c_int * 8), ("layers_per_block", C.c_int),
        ("attn_levels", C.c_int * 8), ("cross_attention_dim", C.c_int), ("num_heads", C.c_int),
        ("norm_num_groups", C.c_int), ("norm_eps", C.c_float), ("context_len", C.c_int),
        ("weight_dtype", C.c_int), ("fp8_act_scale_norm", C.c_float), ("fp8_act_scale_ff", C.c_float),
        ("time_cond_proj_dim", C.c_int),
        ("ip_adapter_tokens", C.c_int), ("ip_adapter_embed_dim", C.c_int),
    ]


class SdUnetConfigFull(SdUnetConfig):
    """``sd_unet_config`` as the library reads it today: the fields above, then what was appended after the IP-Adapter
    (a ctypes subclass lays its fields out behind its base's).  Every entry point takes THIS type: the shorter base would be
    read past its end."""
    _fields_ = [
        ("num_heads_per_level", C.c_int * 8),       # head count per level; all zeros = num_heads at every level
    ]


DTYPE_BF16, DTYPE_FP8_E4M3 = 0, 1
DTYPES = {"bf16": DTYPE_BF16, "fp8": DTYPE_FP8_E4M3, "fp8_e4m3": DTYPE_FP8_E4M3}


class SdClipConfig(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_int), ("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int),
        ("intermediate_size", C.c_int), ("max_positions", C.c_int), ("layer_norm_eps", C.c_float),
        ("hidden_act", C.c_int),            # 0 = quick_gelu, 1 = gelu (exact); appended: the seven-value form leaves it 0
    ]


class SdClipVisionConfig(C.Structure):
    _fields_ = [
        ("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int), ("intermediate_size", C.c_int),
        ("image_size", C.c_int), ("patch_size", C.c_int), ("projection_dim", C.c_int), ("layer_norm_eps", C.c_float),
        ("hidden_act", C.c_int),            # 0 = quick_gelu, 1 = gelu (exact); appended: the eight-value form leaves it 0
    ]


class SdImageRewardConfig(C.Structure):
    _fields_ = [
        ("vision_hidden_size", C.c_int), ("vision_num_layers", C.c_int), ("vision_num_heads", C.c_int),
        ("vision_intermediate_size", C.c_int), ("image_size", C.c_int), ("patch_size", C.c_int),
        ("vision_layer_norm_eps", C.c_float),
        ("vocab_size", C.c_int), ("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int),
        ("intermediate_size", C.c_int), ("max_positions", C.c_int), ("layer_norm_eps", C.c_float), ("hidden_act", C.c_int),
        ("position_embedding_absolute", C.c_int), ("max_text_len", C.c_int), ("reward_mean", C.c_float), ("reward_std", C.c_float),
    ]


class SdHipError(RuntimeError):
    pass


def declared_symbols() -> list:
    """Every function name include/sd_hip.h declares (used by the CPU export test)."""
    src = open(HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", src)))


_vp, _i, _ll, _f = C.c_void_p, C.c_int, C.c_longlong, C.c_float
_SIGS = {
    "sd_last_error": (C.c_char_p, []),
    "sd_abi_version": (_i, []),
    "sd_unet_create": (_i, [C.POINTER(SdUnetConfigFull), C.POINTER(_vp)]),
    "sd_unet_destroy": (None, [_vp]),
    "sd_unet_num_params": (_i, [_vp]),
    "sd_unet_param_info": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_ll), C.POINTER(_i)]),
    "sd_unet_load_param": (_i, [_vp, C.c_char_p, _vp, _ll]),
    "sd_unet_finalize": (_i, [_vp]),
    "sd_unet_debug_packed": (_ll, [_vp, C.c_char_p, _vp, _ll]),
    "sd_unet_calibrate_fp8": (_i, [_vp, _vp, _vp, _i, _i, _f, _f, _vp, _ll]),
    "sd_unet_fp8_scale_count": (_i, [_vp]),
    "sd_unet_fp8_scale_info": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_f), C.POINTER(_f)]),
    "sd_unet_set_fp8_scale": (_i, [_vp, C.c_char_p, _f]),
    "sd_unet_workspace_bytes": (_ll, [_vp, _i, _i]),
    "sd_unet_set_context": (_i, [_vp, _vp, _vp, _i, _i, _vp, _ll]),
    "sd_unet_set_timestep_cond": (_i, [_vp, _vp, _vp]),
    "sd_unet_forward": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _ll, _i, _i]),
    "sd_unet_workspace_bytes_hw": (_ll, [_vp, _i, _i, _i, _i]),
    "sd_unet_set_context_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _ll]),
    "sd_unet_forward_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _ll, _i, _i]),
    "sd_unet_forward_profiled": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _ll, _i, _i, C.POINTER(C.c_double),
                                      C.POINTER(_ll), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sd_unet_forward_op_times": (_ll, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _ll, _i, _i, C.c_char_p, _ll]),
    "sd_vae_create": (_i, [C.POINTER(SdUnetConfigFull), C.POINTER(_vp)]),
    "sd_vae_decode": (_i, [_vp, _vp, _vp, _i, _f, _vp, _vp, _ll]),
    "sd_vae_decode_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _ll]),
    "sd_vae_encoder_create": (_i, [C.POINTER(SdUnetConfigFull), C.POINTER(_vp)]),
    "sd_vae_encode_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _ll]),
    "sd_vae_posterior_sample": (_i, [_vp, _vp, _vp, _f, _vp, _i, _ll]),
    "sd_taesd_decoder_create": (_i, [C.POINTER(_vp)]),
    "sd_taesd_encoder_create": (_i, [C.POINTER(_vp)]),
    "sd_taesd_decode_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _ll]),
    "sd_taesd_encode_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _ll]),
    "sd_op_conv64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_op_conv64_pack": (_ll, [_vp, _vp]),
    "sd_op_taesd_entry": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_op_taesd_exit": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_clip_create": (_i, [C.POINTER(SdClipConfig), C.POINTER(_vp)]),
    "sd_clip_encode": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _ll]),
    "sd_clip_create_projected": (_i, [C.POINTER(SdClipConfig), _i, _i, C.POINTER(_vp)]),
    "sd_clip_text_embeds_workspace_bytes": (_ll, [_vp, _i]),
    "sd_clip_text_embeds": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _ll]),
    "sd_clip_vision_create": (_i, [C.POINTER(SdClipVisionConfig), C.POINTER(_vp)]),
    "sd_clip_vision_workspace_bytes": (_ll, [_vp, _i, _i, _i]),
    "sd_clip_vision_encode": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _ll]),
    "sd_clip_score": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "sd_image_reward_create": (_i, [C.POINTER(SdImageRewardConfig), C.POINTER(_vp)]),
    "sd_image_reward_workspace_bytes": (_ll, [_vp, _i, _i, _i]),
    "sd_image_reward_score": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _ll]),
    "sd_op_bert_attention": (_i, [_vp, _vp, _ll, _vp, _vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i]),
    "sd_op_reward_head": (_i, [_vp, _vp, _ll, _vp, _vp, _f, _f, _i, _i, _vp, _vp]),
    "sd_clip_resize_taps": (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    "sd_op_vit_attention": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_clip_preprocess": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "sd_op_clip_embed": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_activation": (_i, [_vp, _vp, _ll, _i]),
    "sd_op_pool_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sd_op_vit_embed": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i]),
    "sd_op_xattn_expand": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f]),
    "sd_op_transpose_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_retile32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_xattn_fold": (_i, [_vp] * 11 + [_i] * 5),
    "sd_op_ip_fold": (_i, [_vp] * 7 + [_i] * 4 + [_f]),
    "sd_inception_create": (_i, [C.POINTER(_vp)]),
    "sd_inception_destroy": (None, [_vp]),
    "sd_inception_num_convs": (_i, [_vp]),
    "sd_inception_conv_info": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_ll)]),
    "sd_inception_load_conv": (_i, [_vp, C.c_char_p, _vp, _ll, _vp, _i]),
    "sd_inception_finalize": (_i, [_vp]),
    "sd_inception_workspace_bytes": (_ll, [_vp, _i, _i]),
    "sd_inception_features": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _ll]),
    "sd_fid_accumulate": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "sd_op_inception_conv": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "sd_op_maxpool3x3": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i]),
    "sd_op_avgpool3x3": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "sd_op_global_mean": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "sd_op_inception_resize": (_i, [_vp, _vp, _i, _i, _i, _vp, _i]),
    "sd_unet_debug_tensor": (_i, [_vp, _vp, C.c_char_p, _vp, _ll, _vp, _i, _i]),
    "sd_sched_step": (_i, [_vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _ll]),
    "sd_cfg_rescale_factors": (_i, [_vp, _vp, _i, _ll, _f, _f, _vp]),
    "sd_sched_step_rescaled": (_i, [_vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _ll, _vp, _ll]),
    "sd_sched_step_inpaint": (_i, [_vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _ll, _vp, _ll,
                                   _vp, _vp, _vp, _f, _f, _ll]),
    "sd_sched_step_pc": (_i, [_vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _ll, _vp, _ll,
                              _vp, _vp, _vp, _f, _f, _ll]),
    "sd_inpaint_prepare": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i]),
    "sd_unet_set_inpaint_cond_hw": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i]),
    "sd_unet_set_ip_adapter_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _ll]),
    "sd_op_ip_xattn": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _ll, _i, _i, _i, _i]),
    "sd_controlnet_create": (_i, [C.POINTER(SdUnetConfigFull), C.POINTER(_i), C.POINTER(_vp)]),
    "sd_controlnet_residual_bytes_hw": (_ll, [_vp, _i, _i, _i]),
    "sd_controlnet_set_cond_hw": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "sd_controlnet_forward_hw": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _ll]),
    "sd_unet_set_control_residuals_hw": (_i, [_vp, _vp, _f, _i, _i, _i]),
    "sd_op_conv_in_add": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_residual_add": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _f]),
    "sd_op_conv_in_cond": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_gemm": (_i, [_vp, _vp, _ll, _vp, _ll, _i, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _i]),
    "sd_op_gemm_tile_rows": (_i, [_i, _i, _i]),
    "sd_op_gemm_splitk": (_i, [_i, _i, _i, _i]),
    "sd_op_gemm_batched": (_i, [_vp, _vp, _ll, _vp, _ll, _i, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _i]),
    "sd_op_gemm_batched_softmax_ln": (_i, [_vp, _vp, _ll, _vp, _ll, _i, _vp, _ll, _i, _i, _i, _i, _vp, _i, _vp, _vp, _f]),
    "sd_op_conv3x3": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "sd_op_conv3x3_shortcut": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_op_conv3x3_shortcut_groupnorm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i,
                                              _vp, _vp, _vp, _i, _f, _i]),
    "sd_op_conv3x3_down_asym": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_op_conv3x3_ablate": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "sd_op_conv3x3_upsample_subpixel": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_op_conv3x3_upsample_subpixel_groupnorm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _i]),
    "sd_op_groupnorm": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _i]),
    "sd_op_conv3x3_groupnorm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _i]),
    "sd_op_conv3x3_splitk": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "sd_op_conv3x3_kernel": (_i, [_i, _i, _i, _i, _i, _i, _i, _i]),
    "sd_op_softmax_rows": (_i, [_vp, _vp, _ll, _i, _f]),
    "sd_op_layernorm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f]),
    "sd_op_attention": (_i, [_vp, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _f]),
    "sd_op_gemm_qkv_headmajor": (_i, [_vp, _vp, _ll, _vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_attention_headmajor": (_i, [_vp, _vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _f]),
    "sd_op_clip_attention": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_conv_in": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_op_conv_out": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_op_time_embedding": (_i, [_vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i]),
    "sd_op_timestep_cond": (_i, [_vp, _f, _vp, _vp, _vp, _vp, _i, _i]),
    "sd_op_ln_partials": (_i, [_i, _i, _i]),
    "sd_op_gemm_rowstats": (_i, [_vp, _vp, _ll, _vp, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _vp]),
    "sd_op_gemm_plan": (_i, [_vp, _vp, _ll, _vp, _ll, _i, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _f,
                            _vp, _i]),
    "sd_op_gemm_ln": (_i, [_vp, _vp, _ll, _vp, _vp, _vp, _vp, _i, _f, _vp, _ll, _i, _i, _i, _i]),
    "sd_op_xattn_fused_rowstats": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sd_op_xattn_fused": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "sd_op_xattn_fused_ln": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _ll, _vp, _f, _vp]),
    "sd_op_xattn_fused_stamps": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sd_op_gemm_fp8": (_i, [_vp, _vp, _ll, _vp, _vp, _f, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _f]),
    "sd_op_conv3x3_fp8": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "sd_op_groupnorm_fp8": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _f]),
    "sd_op_layernorm_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f]),
    "sd_op_quantize_fp8": (_i, [_vp, _vp, _vp, _ll, _i, _i, _f]),
    "sd_op_amax_e4m3": (_i, [_vp, _vp, _ll, _vp]),
    "sd_unet_set_tome": (_i, [_vp, C.c_double, _i]),
    "sd_unet_tome_block_count_hw": (_i, [_vp, _i, _i]),
    "sd_unet_tome_block_info_hw": (_i, [_vp, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_ll)]),
    "sd_unet_set_tome_choice_hw": (_i, [_vp, _vp, _vp, _ll, _i, _i]),
    "sd_unet_tome_matching_hw": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "sd_op_tome_match": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sd_op_tome_select": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "sd_op_tome_merge": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i]),
    "sd_op_tome_unmerge": (_i, [_vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "sd_unet_set_freeu": (_i, [_vp, _f, _f, _f, _f]),
    "sd_unet_disable_freeu": (_i, [_vp]),
    "sd_unet_plan_count": (_i, [_vp]),
    "sd_unet_option_name": (C.c_char_p, [_i]),
    "sd_unet_option_conflict": (C.c_char_p, [_i, _i]),
    "sd_op_freeu": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f]),
    "sd_unet_tgate_bytes_hw": (_ll, [_vp, _i, _i, _i]),
    "sd_unet_tgate_block_info_hw": (_i, [_vp, _i, _i, _i, _i, C.POINTER(_ll), C.POINTER(_ll), C.POINTER(_i)]),
    "sd_unet_set_tgate_hw": (_i, [_vp, _i, _vp, _ll, _i, _i, _i]),
    "sd_op_tgate_capture": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i]),
    "sd_op_tgate_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _i]),
    "sd_unet_set_hypertile": (_i, [_vp, _i, _i]),
    "sd_unet_hypertile_block_count_hw": (_i, [_vp, _i, _i]),
    "sd_unet_hypertile_block_info_hw": (_i, [_vp, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "sd_hypertile_check": (_i, [_i, _i, _i, _i, _i, _i, _ll]),
    "sd_op_hypertile_gather": (_i, [_vp, _vp, _ll, _vp, _i, _i, _i, _i, _i, _i]),
    "sd_op_hypertile_scatter": (_i, [_vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i]),
    "sd_unet_set_pag": (_i, [_vp, _ll]),
    "sd_unet_pag_block_count": (_i, [_vp]),
    "sd_pag_identity_check": (_i, [_ll, _ll, _ll, _i, _i, _ll, _i]),
    "sd_op_pag_identity": (_i, [_vp, _vp, _ll, _i, _vp, _ll, _ll, _ll, _i, _i]),
    "sd_sched_step_pag": (_i, [_vp, _vp, _i, _f, _f] + [_vp] * 8 + [C.POINTER(_f), _ll, _vp, _ll, _vp, _vp, _vp, _f, _f, _ll]),
    "sd_sched_step_pc_pag": (_i, [_vp, _vp, _i, _f, _f] + [_vp] * 9 + [C.POINTER(_f), _ll, _vp, _ll, _vp, _vp, _vp, _f, _f, _ll]),
    "sd_cfg_rescale_factors_pag": (_i, [_vp, _vp, _i, _ll, _f, _f, _f, _vp]),
    "sd_unet_set_sag": (_i, [_vp, _i]),
    "sd_unet_set_sag_buffer": (_i, [_vp, _vp, _ll]),
    "sd_sag_mass_check": (_i, [_i, _i, _i, _i, _ll, _i]),
    "sd_op_sag_attn_mass": (_i, [_vp, _vp, _vp, _ll, _vp, _i, _i, _i, _i, _i]),
    "sd_op_sag_degrade": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(_f), _vp, _i, _i, _i]),
    "sd_sched_step_sag": (_i, [_vp, _vp, _i, _f, _f] + [_vp] * 8 + [C.POINTER(_f), _ll, _vp, _ll, _vp, _vp, _vp, _f, _f, _ll]),
    "sd_sched_step_pc_sag": (_i, [_vp, _vp, _i, _f, _f] + [_vp] * 9 + [C.POINTER(_f), _ll, _vp, _ll, _vp, _vp, _vp, _f, _f, _ll]),
}


def _open(path: str, missing_message: str) -> C.CDLL:
    if not os.path.exists(path):
        raise SdHipError(missing_message)
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


def load() -> C.CDLL:
    """Load libsdhip.so (RTLD_GLOBAL not needed); raises SdHipError if it is not built."""
    global _lib
    if _lib is None:
        _lib = _open(LIB_PATH, f"{LIB_PATH} is missing: build it with `python -m sonicdiffusionbayeslab_amd.build` "
                               "(or __graft_entry__.build()).  There is no CPU/PyTorch fallback for the hot path.")
    return _lib


def load_ablate() -> C.CDLL:
    """libsdhip_ablate.so: a SECOND, independent instance of the library built with -DSD_ABLATE (its own globals).  Never
    used by the product path; raises if it is not built."""
    global _ablate
    if _ablate is None:
        _ablate = _open(ABLATE_LIB_PATH, f"{ABLATE_LIB_PATH} is missing: build it with `python -m sonicdiffusionbayeslab_amd.build`")
    return _ablate


def check(rc: int, what: str = "libsdhip call", lib: Optional[C.CDLL] = None) -> None:
    if rc != 0:
        msg = (lib or load()).sd_last_error()
        raise SdHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def ptr(t) -> Optional[int]:
    """Device/host pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
