"""ctypes binding of libthinkdiff_hip.so (the C ABI in include/thinkdiff_hip.h).

torch is used here only as the owner of device memory and streams: every call passes raw device
pointers + sizes to the C ABI.  There is deliberately NO fallback: if the library is missing the
import of any op raises, so a GPU run can never silently take an eager/CPU path.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# TD_HIP_LIB: another build of the same library (A/B timing of two builds on one box); never a different implementation
LIB_PATH = os.environ.get("TD_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libthinkdiff_hip.so")

ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU, ACT_QUICK_GELU = 0, 1, 2, 3, 4

_lib = None


class ThinkDiffHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raise loudly when the .so is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ThinkDiffHipError(
                f"{LIB_PATH} not found: build it with `make -C thinkdiff-mlre_amd` "
                "(or __graft_entry__.build()); there is no fallback path")
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.td_last_error.restype = ctypes.c_char_p
        _declare(_lib)
    return _lib


def _declare(L):
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    sig = {
        "td_abi_version": [],
        "td_linear_bf16": [vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, i64, vp],
        "td_linear_split_bf16": [vp, i64, vp, vp, vp, i64, i32, vp, i64, i32, i32, i32, i32, i32, vp],
        "td_linear_splitk_bf16": [vp, i64, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32, vp, i64, i32, i32, vp, vp, i64, f32, vp],
        "td_linear_grouped2_bf16": [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, i32, vp],
        "td_gemm_plan_query": [i32, i32, i32, i32, i32],
        "td_linear_drain_bf16": [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp, i64, i32, i32, i32, vp],
        "td_norm_rows_bf16": [vp, i64, vp, i64, i32, i32, i32, f32, vp, i32, vp, vp, vp, vp, vp],
        "td_qk_norm_rope_bf16": [vp, i64, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, f32, i32, vp],
        "td_qk_norm_rope_premul_bf16": [vp, i64, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, f32, i32, f32, vp],
        "td_temb_combine_silu_bf16": [vp, vp, vp, i32, i32, vp, vp, vp],
        "td_copy_cols_bf16": [vp, i64, vp, i64, i32, i32, vp],
        "td_flux_rope_table": [vp, i32, vp, ctypes.c_double, vp, vp, vp],
        "td_timestep_sincos": [vp, i32, vp, vp],
        "td_euler_step_bf16": [vp, vp, f32, i64, vp],
        "td_flux_inpaint_step_bf16": [vp, vp, vp, vp, vp, f32, f32, i64, vp],
        "td_flux_cfg_step_bf16": [vp, vp, vp, f32, f32, i64, vp],
        "td_flux_residual_inject_bf16": [vp, i64, vp, i64, i32, i32, f32, vp],
        "td_block_cache_head_bf16": [vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, vp, vp, vp],
        "td_block_cache_tail_bf16": [vp, i64, vp, i64, vp, i64, i32, i32, vp],
        "td_redux_compose_bf16": [vp, i64, i32, vp, i64, i32, ctypes.POINTER(f32), i32, i32, vp, i64, vp],
        "td_flux_set_block_cache": [vp, i32, f32],
        "td_flux_set_block_cache_schedule": [vp, vp, i32],
        "td_flux_block_cache_reset": [vp],
        "td_flux_block_cache_stats": [vp, i32, vp, vp, vp],
        "td_flux_controlnet_create": [vp, i32, i32, i32, i32, vp],
        "td_flux_controlnet_set_mode": [vp, i32],
        "td_flux_controlnet_set_condition": [vp, vp, vp],
        "td_flux_controlnet_forward": [vp, vp, i32, vp],
        "td_flux_controlnet_samples": [vp, vp, vp, vp, vp, vp, vp],
        "td_flux_controlnet_read_sample": [vp, i32, vp, vp],
        "td_flux_attach_controlnet": [vp, vp],
        "td_flux_set_controlnet_scales": [vp, vp, i32],
        "td_flux_attach_controlnets": [vp, vp, i32],
        "td_flux_set_controlnet_scales_at": [vp, i32, vp, i32],
        "td_flux_attached_controlnets": [vp, vp],
        "td_flux_residual_inject_multi_bf16": [vp, i64, vp, vp, vp, i32, i32, i32, vp],
        "td_flux_inpaint_mask": [vp, i32, i32, i32, i32, vp, vp],
        "td_flux_pack_latents": [vp, vp, i32, i32, i32, i32, f32, f32, vp],
        "td_cls_avgpool2_bf16": [vp, vp, i32, i32, vp],
        "td_fill_normal_bf16": [vp, i64, ctypes.c_uint64, f32, f32, vp],
        "td_fill_normal_from_bf16": [vp, i64, ctypes.c_uint64, f32, f32, i64, vp],
        "td_aligner_mlp2x_bf16": [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, f32, i32, vp, vp, i64, vp],
        "td_flux_create": [vp, i32, i32, i32, vp],
        "td_flux_num_params": [vp],
        "td_flux_param_info": [vp, i32, ctypes.c_char_p, i32, vp],
        "td_flux_load_param": [vp, ctypes.c_char_p, vp, i64, vp],
        "td_flux_init_random": [vp, ctypes.c_uint64, f32, vp],
        "td_flux_set_precision": [vp, i32, vp],
        "td_flux_set_fp8_gemms": [vp, ctypes.c_uint],
        "td_flux_set_act_scales": [vp, i32],
        "td_flux_set_smoothing": [vp, i32],
        "td_flux_set_attention": [vp, i32],
        "td_flux_prepared_shape": [vp, vp, vp, vp, vp],
        "td_flux_input_shape": [vp, vp, vp, vp],
        "td_flux_set_channel_condition": [vp, vp, vp],
        "td_flux_set_reference_tokens": [vp, vp, i32, vp, vp],
        "td_flux_reference_tokens": [vp, vp],
        "td_flux_denoise_cfg": [vp, vp, vp, vp, i32, f32, vp],
        "td_flux_fill_condition": [vp, vp, vp, i32, i32, i32, f32, f32, i32, vp, vp],
        "td_vae_encode_masked": [vp, vp, i32, vp, i32, i32, i32, vp, vp],
        "td_vae_image_to_nhwc_masked_bf16": [vp, i32, vp, i32, i32, i32, vp, i32, vp],
        "td_vae_output_shape": [vp, i32, i32, vp, vp, vp],
        "td_lora_pack_bf16": [vp, vp, i32, i32, i32, vp, vp],
        "td_lora_merge_bf16": [vp, vp, i32, i32, i32, vp, vp, vp, vp],
        "td_flux_read_param": [vp, ctypes.c_char_p, vp, i64, vp],
        "td_flux_param_shape": [vp, ctypes.c_char_p, vp, vp],
        "td_flux_lora_load": [vp, ctypes.c_char_p, ctypes.c_char_p, vp, vp, i32, f32, vp],
        "td_flux_lora_set_adapters": [vp, vp, vp, i32, vp],
        "td_flux_lora_delete": [vp, ctypes.c_char_p, vp],
        "td_flux_lora_clear": [vp, vp],
        "td_flux_lora_info": [vp, vp, vp, vp],
        "td_ip_attention_bf16": [vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, vp, f32, f32, i32, vp],
        "td_flux_ip_adapter_add": [vp, i32, i32, vp],
        "td_flux_ip_adapter_load_param": [vp, i32, ctypes.c_char_p, vp, i64, vp],
        "td_flux_ip_adapter_remove": [vp, i32],
        "td_flux_set_ip_adapter_scale": [vp, i32, vp, i32],
        "td_flux_ip_adapter_info": [vp, i32, vp, vp, vp, vp, vp],
        "td_flux_set_ip_image_embeds": [vp, i32, vp, i32, vp],
        "td_flux_ip_read": [vp, i32, i32, i32, vp, vp],
        "td_flux_ip_widths": [vp, vp, vp],
        "td_flux_fork": [vp, vp],
        "td_flux_denoise_multi": [vp, vp, i32, vp, i32, vp],
        "td_flux_denoise_multi_inpaint": [vp, vp, i32, vp, i32, vp, vp, vp, vp],
        "td_flux_set_condition": [vp, vp, i32, vp, vp, vp, i32, vp],
        "td_flux_set_timesteps": [vp, vp, i32, f32, vp],
        "td_flux_forward": [vp, vp, i32, vp, vp],
        "td_flux_denoise": [vp, vp, vp, i32, vp],
        "td_flux_denoise_inpaint": [vp, vp, vp, i32, vp, vp, vp, vp],
        "td_flux_trace_begin": [vp, i32],
        "td_flux_trace_end": [vp, vp, vp, vp, vp],
        "td_attention_set_variant": [i32],
        "td_attention_decode_set_group": [i32],
        "td_quant_rows_fp8": [vp, i64, vp, i64, vp, i32, i32, vp],
        "td_linear_fp8": [vp, i64, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, i64, i32, vp],
        "td_quant_rows_int8": [vp, i64, vp, i64, vp, i32, i32, vp],
        "td_linear_int8": [vp, i64, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, i64, i32, vp],
        "td_norm_rows_quant_fp8": [vp, i64, vp, i64, vp, i32, i32, i32, f32, vp, i32, vp, vp, vp, vp, vp],
        "td_norm_rows_quant8": [vp, i64, vp, i64, vp, i32, i32, i32, f32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp],
        "td_quant_rows8": [vp, i64, vp, i64, vp, i32, i32, i32, vp, vp, vp],
        "td_col_amax_bf16": [vp, i64, i32, i32, vp, vp],
        "td_smooth_factors": [vp, vp, i32, vp, vp, vp, vp],
        "td_q8_scales_from_amax": [vp, vp, vp, i64, f32, vp],
        "td_ext_cols_int8": [vp, i64, i32, i32, vp, i32, vp],
        "td_linear_int8_q8": [vp, i64, i64, i32, i32, i32, i32, vp],
        "td_linear_split_int8_q8": [vp, i64, i64, vp, i64, i32, i32, i32, i32, i32, i32, vp],
        "td_linear_grouped2_int8_q8": [vp, vp, i64, i64, i32, i32, i32, i32, vp],
        "td_attention_q8": [vp, i64, vp, vp, i64, vp, i64, vp, vp, i32, i32, i32, f32, i32, vp, i32, f32, vp],
        "td_attention_fp8_q8": [vp, i64, vp, vp, i64, vp, i64, vp, vp, i32, i32, i32, f32, vp, vp],
        "td_layernorm_bf16": [vp, i64, vp, i64, i32, i32, i32, f32, vp, vp, vp],
        "td_add_rows_bf16": [vp, vp, vp, i32, i32, i32, vp],
        "td_glu_mul_bf16": [vp, vp, i32, i32, i32, vp],
        "td_attention_bias_bf16": [vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, i32, f32, i32, vp, vp],
        "td_attention_varlen_bf16": [vp, i64, vp, vp, i64, vp, i64, vp, i32, i32, i32, i32, f32, vp],
        "td_attention_segments_bf16": [vp, i64, vp, vp, i64, vp, i64, vp, i32, i32, i32, i32, f32, i32, vp],
        "td_attention_prefix_segments_bf16": [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp],
        "td_rope_half_bf16": [vp, i64, i32, i32, i32, i32, vp, vp, vp],
        "td_vision_rope_table": [vp, i32, i32, f32, vp, vp, vp],
        "td_patchify_bf16": [vp, i32, i32, i32, i32, i32, vp, i32, vp],
        "td_qwen2_patchify_u8": [vp, i32, i32, vp, i32, i32, i32, vp, i32, vp],
        "td_cast_pad_rows_bf16": [vp, i32, i32, i32, vp, i32, vp],
        "td_resize_coeffs": [i32, i32, i32, vp, vp, vp],
        "td_image_resize_u8": [vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp],
        "td_image_lut_chw_f32": [vp, i32, i32, i32, vp, vp, vp],
        "td_vae_create": [vp, i32, i32, vp],
        "td_vae_num_params": [vp],
        "td_vae_param_info": [vp, i32, ctypes.c_char_p, i32, vp],
        "td_vae_load_param": [vp, ctypes.c_char_p, vp, i64, vp],
        "td_vae_init_random": [vp, ctypes.c_uint64, f32, vp],
        "td_vae_decode": [vp, vp, i32, i32, f32, f32, vp, vp, vp],
        "td_conv3x3_nhwc_bf16": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
        "td_conv3x3_pack_weight": [vp, vp, i32, i32, i32, i32, vp],
        "td_conv3x3_s2_nhwc_bf16": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
        "td_vae_latents_to_nhwc_bf16": [vp, vp, i32, i32, i32, i32, f32, f32, vp],
        "td_vae_image_finalize": [vp, i32, i32, vp, vp, vp],
        "td_vae_enc_create": [vp, i32, i32, vp],
        "td_vae_enc_num_params": [vp],
        "td_vae_enc_param_info": [vp, i32, ctypes.c_char_p, i32, vp],
        "td_vae_enc_load_param": [vp, ctypes.c_char_p, vp, i64, vp],
        "td_vae_enc_init_random": [vp, ctypes.c_uint64, f32, vp],
        "td_vae_enc_output_shape": [vp, i32, i32, vp, vp, vp],
        "td_vae_encode": [vp, vp, i32, i32, i32, vp, vp],
        "td_vae_latents_from_moments": [vp, vp, vp, f32, f32, f32, i32, i32, i32, vp, vp],
        "td_vae_image_to_nhwc_bf16": [vp, i32, i32, i32, vp, i32, vp],
        "td_linear_f32out_bf16": [vp, i64, vp, vp, vp, i64, i32, i32, i32, vp],
        "td_groupnorm_nhwc_bf16": [vp, vp, i32, i32, i32, f32, vp, vp, i32, vp, vp],
        "td_groupnorm_workspace_floats": [],
        "td_softmax_rows_f32_bf16": [vp, vp, i32, i32, f32, vp],
        "td_softmax_rows_strided_f32_bf16": [vp, vp, i32, i32, i32, f32, vp],
        "td_qwen2_create": [vp, i32, vp],
        "td_qwen2_num_params": [vp],
        "td_qwen2_param_info": [vp, i32, ctypes.c_char_p, i32, vp],
        "td_qwen2_load_param": [vp, ctypes.c_char_p, vp, i64, vp],
        "td_qwen2_init_random": [vp, ctypes.c_uint64, f32, vp],
        "td_qwen2_forward": [vp, vp, vp, vp, i32, i32, vp, vp, vp],
        "td_qwen2_embed_tokens": [vp, vp, vp, i32, vp],
        "td_qwen2_forward_slot": [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp],
        "td_qwen2_set_slots": [vp, i32],
        "td_qwen2_set_fused_rope": [vp, i32],
        "td_qwen2_create_slots": [vp, i32, i32, vp],
        "td_qwen2_create_ex": [vp, i32, i32, i32, vp],
        "td_qwen2_prefill_batch": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "td_qwen2_prefill_batch_at": [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "td_qwen2_prefill_packed": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "td_qwen2_prefill_packed_slots": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "td_qwen2_prefill_packed_prefix_slots": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "td_qwen2_slot_capacity": [vp],
        "td_qwen2_move_slot": [vp, i32, i32, i32, vp],
        "td_qwen2_fork_slot": [vp, i32, vp, i32, i32, vp],
        "td_kv_fork_rows": [vp, i32, i32, vp, i32, i32, vp],
        "td_kv_gather_rows": [vp, i32, i32, vp, vp, vp, vp],
        "td_qwen2_gather_slots": [vp, i32, vp, vp, vp, vp],
        "td_beam_select": [vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "td_attention_verify": [vp, i64, vp, vp, i64, i64, vp, vp, vp, vp, i64, i64, vp, i64, i32, vp, vp, vp, vp, i32, i32, f32, vp],
        "td_attention_verify_set_form": [i32],
        "td_attention_verify_ex": [vp, i64, vp, vp, i64, i64, vp, vp, vp, vp, i64, i64, vp, i64, i32, vp, vp, vp, vp, i32, i32, f32, i32, i32, vp],
        "td_qwen2_verify_batch_slots": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "td_spec_accept": [vp, vp, vp, vp, i32, vp, vp, vp],
        "td_qwen2_decode_batch": [vp, i32, vp, vp, vp, vp, vp, vp],
        "td_qwen2_decode_batch_slots": [vp, i32, vp, vp, vp, vp, vp, vp, vp],
        "td_qwen2_quantize_weights": [vp, i32, vp],
        "td_qwen2_set_weight_stream": [vp, i32],
        "td_qwen2_weight_info": [vp, vp, vp, vp, vp],
        "td_qwen2_create_kv": [vp, i32, i32, i32, i32, vp],
        "td_qwen2_kv_info": [vp, vp, vp, vp],
        "td_qwen2_read_kv": [vp, i32, i32, i32, i32, vp, vp],
        "td_kv_quant_rows_e4m3": [vp, i64, vp, i64, vp, i64, vp, i32, i32, vp, vp],
        "td_kv_dequant_rows_e4m3": [vp, i64, vp, i64, vp, i64, i32, i32, vp],
        "td_attention_decode_kv8": [vp, i64, i64, vp, vp, i64, i64, vp, vp, i64, i64, vp, i64, i64, i32, i32, vp, i32, i32, f32, vp],
        "td_quant_weight_rows_e4m3": [vp, i64, vp, vp, vp, i32, i32, vp],
        "td_linear_w8_bf16": [vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, i64, vp],
        "td_linear_split_w8_bf16": [vp, i64, vp, vp, vp, vp, i64, i32, vp, i64, i32, i32, i32, i32, i32, vp],
        "td_linear_glu_bf16": [vp, i64, vp, vp, i64, i32, i32, i32, vp],
        "td_linear_glu_w8_bf16": [vp, i64, vp, vp, vp, i64, i32, i32, i32, vp],
        "td_quant_weight_rows_mxfp4": [vp, i64, vp, vp, vp, i32, i32, vp],
        "td_dequant_rows_mxfp4": [vp, vp, vp, i64, i32, i32, vp],
        "td_linear_w4_bf16": [vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, i64, vp],
        "td_linear_split_w4_bf16": [vp, i64, vp, vp, vp, vp, i64, i32, vp, i64, i32, i32, i32, i32, i32, vp],
        "td_linear_glu_w4_bf16": [vp, i64, vp, vp, vp, i64, i32, i32, i32, vp],
        "td_repack_int4": [i32, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp],
        "td_dequant_rows_int4": [vp, vp, vp, i32, vp, i64, i32, i32, vp],
        "td_linear_i4_bf16": [vp, i64, vp, vp, vp, i32, vp, vp, i64, i32, i32, i32, i32, vp, vp, i64, vp],
        "td_linear_split_i4_bf16": [vp, i64, vp, vp, vp, i32, vp, vp, i64, i32, vp, i64, i32, i32, i32, i32, i32, vp],
        "td_linear_glu_i4_bf16": [vp, i64, vp, vp, vp, i32, vp, i64, i32, i32, i32, vp],
        "td_qwen2_load_param_int4": [vp, ctypes.c_char_p, vp, vp, vp, i32, vp],
        "td_qwen2_set_int4_routing": [vp, i32],
        "td_embed_gather_bf16": [vp, vp, vp, i32, i32, i32, vp],
        "td_silu_mul_bf16": [vp, vp, i32, i32, vp],
        "td_mrope_table": [vp, i32, vp, f32, i32, vp, vp, vp],
        "td_attention_bf16": [vp, i64, i64, vp, vp, i64, i64, vp, i64, i64, i32, i32, i32, i32, i32, i32, f32, i32, vp],
        "td_attention_fp8": [vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, f32, vp, vp],
        "td_attention_joint_prescaled_bf16": [vp, i64, vp, vp, i64, vp, i64, i32, i32, f32, vp],
        "td_attention_fp8_qk_rope": [vp, i64, i32, i32, i32, vp, i64, i32, i32, vp, vp, i32, vp, vp, vp, vp, f32, f32, vp, vp],
        "td_sample_top_p_bf16": [vp, i64, i32, i32, f32, f32, ctypes.c_uint64, ctypes.c_uint64, vp, vp],
        "td_sampler_create": [i32, i32, vp],
        "td_sampler_reset_slot": [vp, i32, vp, i32, vp],
        "td_sampler_read_counts": [vp, i32, vp, vp],
        "td_sampler_read_prompt_mask": [vp, i32, vp, vp],
        "td_sampler_set_counts": [vp, i32, vp, vp],
        "td_sample_rows_bf16": [vp, vp, i64, i32, i32, vp, vp, i32, vp, vp],
        "td_logit_edits_create": [i32, i32, vp],
        "td_logit_edits_reset_slot": [vp, i32, vp],
        "td_logit_edits_set_bias": [vp, i32, vp, vp, i32, vp],
        "td_logit_edits_ban": [vp, i32, vp, i32, i32, vp],
        "td_logit_edits_allow_only": [vp, i32, vp, i32, vp],
        "td_logit_edits_read": [vp, i32, vp, vp, vp],
        "td_sample_rows_edit_bf16": [vp, vp, vp, vp, i64, i32, i32, vp, vp, i32, vp, vp],
        "td_logprobs_rows_bf16": [vp, i64, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp],
        "td_lora_rows_pack_bf16": [vp, vp, i32, i32, i32, vp, vp],
        "td_lora_rows_bf16": [vp, i64, i32, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, ctypes.c_size_t, vp],
        "td_qwen2_lora_enable": [vp, i32, i32],
        "td_qwen2_lora_load": [vp, i32, ctypes.c_char_p, vp, vp, i32, f32, vp],
        "td_qwen2_lora_remove": [vp, i32],
        "td_qwen2_lora_set_slot": [vp, i32, i32],
        "td_qwen2_lora_info": [vp, vp, vp, vp, vp],
    }
    for name, args in sig.items():
        if os.environ.get("TD_HIP_LIB") and not hasattr(L, name):
            continue          # an older build under A/B timing may predate an entry point; the shipped library must export all
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    L.td_flux_destroy.argtypes = [vp]
    L.td_flux_destroy.restype = None
    L.td_vae_destroy.argtypes = [vp]
    L.td_vae_destroy.restype = None
    L.td_vae_enc_destroy.argtypes = [vp]
    L.td_vae_enc_destroy.restype = None
    L.td_qwen2_destroy.argtypes = [vp]
    L.td_qwen2_destroy.restype = None
    if hasattr(L, "td_sampler_destroy"):
        L.td_sampler_destroy.argtypes = [vp]
        L.td_sampler_destroy.restype = None
        L.td_sample_row_size.argtypes = []
        L.td_sample_row_size.restype = ctypes.c_size_t
    if hasattr(L, "td_logit_edits_destroy"):
        L.td_logit_edits_destroy.argtypes = [vp]
        L.td_logit_edits_destroy.restype = None
    L.td_qwen2_weight_stream_launches.argtypes = [vp]
    L.td_qwen2_weight_stream_launches.restype = ctypes.c_int64
    L.td_flux_param_elems.argtypes = [vp]
    L.td_flux_param_elems.restype = ctypes.c_int64
    L.td_lora_packed_bytes.argtypes = [i32, i32, i32]
    L.td_lora_packed_bytes.restype = ctypes.c_size_t
    if hasattr(L, "td_lora_rows_packed_bytes"):
        L.td_lora_rows_packed_bytes.argtypes = [i32, i32, i32]
        L.td_lora_rows_packed_bytes.restype = ctypes.c_size_t
        L.td_lora_rows_workspace_bytes.argtypes = [i32, i32, i32, i32]
        L.td_lora_rows_workspace_bytes.restype = ctypes.c_size_t
    L.td_attention_fp8_workspace_bytes.argtypes = [i32, i32, i32]
    L.td_attention_fp8_workspace_bytes.restype = ctypes.c_size_t
    return sig


def check(status):
    if status != 0:
        raise ThinkDiffHipError(f"libthinkdiff_hip error {status}: {lib().td_last_error().decode()}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda, "thinkdiff_hip ops take device tensors only"
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(t):
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.bfloat16, (t.shape, t.stride(), t.dtype)
    return t.stride(0)


def linear(x, w, bias=None, act=ACT_NONE, gate=None, res=None, out=None):
    """out = act(x @ w.T + bias) * gate + res   (2-D bf16 tensors, row stride may exceed width)."""
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_bf16(ptr(x), _rows(x), ptr(w), ptr(bias), ptr(out), _rows(out), M, N, K, act,
                               ptr(gate), ptr(res), _rows(res) if res is not None else 0, stream_ptr()))
    return out


QWEN2_WEIGHTS_BF16, QWEN2_WEIGHTS_E4M3, QWEN2_WEIGHTS_MXFP4, QWEN2_WEIGHTS_INT4 = 0, 1, 2, 3
INT4_AWQ, INT4_GPTQ, INT4_GPTQ_V2 = 0, 1, 2      # td_repack_int4 layouts; INT4_GPTQ_V2 is a flag on INT4_GPTQ (zero points stored as they are)
INT4_GROUP_SIZES = (32, 64, 128)


def quant_weight_rows_e4m3(w, want_w_hat=True, inplace=False):
    """Weight-only e4m3 quantisation with one power-of-two scale per row (td_quant_weight_rows_e4m3): w bf16 [N, K] (row stride may exceed K) ->
    (q uint8 [N, K], scale fp32 [N] = 2^e_n, w_hat bf16 = q 2^e_n exactly, or None).  inplace: w_hat is written over w."""
    N, K = w.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    scale = torch.empty((N,), dtype=torch.float32, device=w.device)
    w_hat = w if inplace else (torch.empty_like(w) if want_w_hat else None)
    if w_hat is not None:
        assert w_hat.stride(0) == w.stride(0)
    check(lib().td_quant_weight_rows_e4m3(ptr(w), _rows(w), ptr(q), ptr(scale), ptr(w_hat), N, K, stream_ptr()))
    return q, scale, w_hat


QWEN2_KV_BF16, QWEN2_KV_E4M3 = 0, 1


def kv_quant_rows_e4m3(kv, heads, q=None, scale=None, dst_rows=None, want_kv_hat=True, inplace=False):
    """The e4m3 KV-cache format on bf16 rows (td_kv_quant_rows_e4m3): kv [rows, >= heads * 128] -> (q uint8, scale fp32 = 2^e, kv_hat bf16 = q 2^e
    exactly, or None).  q [R, >= heads * 128] / scale [R, >= heads] may be given (views of larger planes) with dst_rows int32 [rows]: row r is then written at
    row dst_rows[r] and no other row is touched.  inplace: kv_hat is written over kv."""
    rows = kv.shape[0]
    assert kv.dim() == 2 and kv.dtype == torch.bfloat16 and kv.stride(1) == 1
    if q is None:
        assert dst_rows is None
        q = torch.empty((rows, heads * 128), dtype=torch.uint8, device=kv.device)
        scale = torch.empty((rows, heads), dtype=torch.float32, device=kv.device)
    assert q.dtype == torch.uint8 and scale.dtype == torch.float32 and q.dim() == 2 and scale.dim() == 2 and q.stride(1) == 1 and scale.stride(1) == 1
    if dst_rows is not None:
        assert dst_rows.dtype == torch.int32 and dst_rows.is_contiguous() and dst_rows.numel() == rows
    kv_hat = kv if inplace else (torch.empty_strided(kv.shape, kv.stride(), dtype=kv.dtype, device=kv.device) if want_kv_hat else None)
    check(lib().td_kv_quant_rows_e4m3(ptr(kv), kv.stride(0), ptr(q), q.stride(0), ptr(scale), scale.stride(0), ptr(kv_hat), rows, int(heads),
                                      ptr(dst_rows), stream_ptr()))
    return q, scale, kv_hat


def kv_dequant_rows_e4m3(q, scale, out=None):
    """bytes [rows, >= heads * 128] + scales [rows, heads] -> bf16 [rows, heads * 128] = q 2^e (td_kv_dequant_rows_e4m3)."""
    assert q.dtype == torch.uint8 and scale.dtype == torch.float32 and q.dim() == 2 and scale.dim() == 2 and q.stride(1) == 1 and scale.stride(1) == 1
    rows, heads = scale.shape
    if out is None:
        out = torch.empty((rows, heads * 128), dtype=torch.bfloat16, device=q.device)
    assert out.dtype == torch.bfloat16 and out.stride(1) == 1
    check(lib().td_kv_dequant_rows_e4m3(ptr(q), q.stride(0), ptr(scale), scale.stride(0), ptr(out), out.stride(0), rows, heads, stream_ptr()))
    return out


def attention_decode_kv8(q, k8, v8, k_scale, v_scale, Hq, Hkv, kv_lens=None, scale=None, out=None):
    """Decode attention over an e4m3 cache (td_attention_decode_kv8): q bf16 [B, >= Hq*128]; k8, v8 uint8 [B, Skv, >= Hkv*128] and k_scale, v_scale fp32
    [B, Skv, >= Hkv] (views into the byte / scale planes; k and v share their strides); kv_lens int32 [B] or None -> out bf16 [B, Hq*128]."""
    B, Skv = k8.shape[0], k8.shape[1]
    assert q.dim() == 2 and q.dtype == torch.bfloat16 and q.stride(1) == 1 and q.shape[0] == B
    for t in (k8, v8):
        assert t.dim() == 3 and t.dtype == torch.uint8 and t.stride(2) == 1
    for t in (k_scale, v_scale):
        assert t.dim() == 3 and t.dtype == torch.float32 and t.stride(2) == 1 and t.shape[:2] == (B, Skv)
    assert k8.stride() == v8.stride() and k_scale.stride() == v_scale.stride()
    if kv_lens is not None:
        assert kv_lens.dtype == torch.int32 and kv_lens.is_contiguous() and kv_lens.numel() == B
    if out is None:
        out = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device=q.device)
    if scale is None:
        scale = 128 ** -0.5
    check(lib().td_attention_decode_kv8(ptr(q), q.stride(0), q.stride(0), ptr(k8), ptr(v8), k8.stride(1), k8.stride(0), ptr(k_scale), ptr(v_scale),
                                        k_scale.stride(1), k_scale.stride(0), ptr(out), out.stride(0), out.stride(0), B, Skv, ptr(kv_lens), Hq, Hkv,
                                        float(scale), stream_ptr()))
    return out


def _w8(x, wq, w_scale):
    M, K = x.shape
    assert wq.dtype == torch.uint8 and wq.dim() == 2 and wq.is_contiguous() and wq.shape[1] == K, (wq.shape, wq.dtype, K)
    assert w_scale.dtype == torch.float32 and w_scale.is_contiguous() and w_scale.numel() == wq.shape[0]
    return M, wq.shape[0], K


def linear_w8(x, wq, w_scale, bias=None, act=ACT_NONE, gate=None, res=None, out=None):
    """linear() with the weight as e4m3 bytes + row scales (the 8-bit weight stream; M <= 64)."""
    M, N, K = _w8(x, wq, w_scale)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_w8_bf16(ptr(x), _rows(x), ptr(wq), ptr(w_scale), ptr(bias), ptr(out), _rows(out), M, N, K, act,
                                  ptr(gate), ptr(res), _rows(res) if res is not None else 0, stream_ptr()))
    return out


def linear_split_w8(x, wq, w_scale, bias, out0, act0, out1, act1, n_split):
    M, N, K = _w8(x, wq, w_scale)
    check(lib().td_linear_split_w8_bf16(ptr(x), _rows(x), ptr(wq), ptr(w_scale), ptr(bias), ptr(out0), _rows(out0), act0,
                                        ptr(out1), _rows(out1), act1, M, N, K, n_split, stream_ptr()))
    return out0, out1


def quant_weight_rows_mxfp4(w, want_w_hat=True, inplace=False):
    """Weight-only OCP MXFP4 quantisation (td_quant_weight_rows_mxfp4): w bf16 [N, K] (K % 32 == 0; row stride may exceed K) -> (packed uint8 [N, K / 2],
    element 2j in the low nibble of byte j; scales uint8 [N, K / 32] = e + 127; w_hat bf16 = q 2^e exactly, or None).  inplace: w_hat is written over w."""
    N, K = w.shape
    packed = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    scales = torch.empty((N, K // 32), dtype=torch.uint8, device=w.device)
    w_hat = w if inplace else (torch.empty_strided(w.shape, w.stride(), dtype=w.dtype, device=w.device) if want_w_hat else None)
    check(lib().td_quant_weight_rows_mxfp4(ptr(w), _rows(w), ptr(packed), ptr(scales), ptr(w_hat), N, K, stream_ptr()))
    return packed, scales, w_hat


def _w4(x, packed, scales):
    M, K = x.shape
    assert packed.dtype == torch.uint8 and packed.dim() == 2 and packed.is_contiguous() and packed.shape[1] * 2 == K, (packed.shape, packed.dtype, K)
    assert scales.dtype == torch.uint8 and scales.is_contiguous() and scales.shape == (packed.shape[0], K // 32), (scales.shape, scales.dtype, K)
    return M, packed.shape[0], K


def dequant_rows_mxfp4(packed, scales, out=None):
    """packed [N, K / 2] + scales [N, K / 32] -> bf16 [N, K] = q 2^e, exactly (td_dequant_rows_mxfp4)."""
    assert packed.dtype == torch.uint8 and scales.dtype == torch.uint8 and packed.dim() == 2 and packed.is_contiguous() and scales.is_contiguous()
    N, K = packed.shape[0], packed.shape[1] * 2
    assert scales.shape == (N, K // 32), (scales.shape, N, K)
    if out is None:
        out = torch.empty((N, K), dtype=torch.bfloat16, device=packed.device)
    assert out.dtype == torch.bfloat16 and out.stride(1) == 1
    check(lib().td_dequant_rows_mxfp4(ptr(packed), ptr(scales), ptr(out), out.stride(0), N, K, stream_ptr()))
    return out


def linear_w4(x, packed, scales, bias=None, act=ACT_NONE, gate=None, res=None, out=None):
    """linear() with the weight as MXFP4 nibbles + block scale bytes (the 4-bit weight stream; M <= 64)."""
    M, N, K = _w4(x, packed, scales)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_w4_bf16(ptr(x), _rows(x), ptr(packed), ptr(scales), ptr(bias), ptr(out), _rows(out), M, N, K, act,
                                  ptr(gate), ptr(res), _rows(res) if res is not None else 0, stream_ptr()))
    return out


def linear_split_w4(x, packed, scales, bias, out0, act0, out1, act1, n_split):
    M, N, K = _w4(x, packed, scales)
    check(lib().td_linear_split_w4_bf16(ptr(x), _rows(x), ptr(packed), ptr(scales), ptr(bias), ptr(out0), _rows(out0), act0,
                                        ptr(out1), _rows(out1), act1, M, N, K, n_split, stream_ptr()))
    return out0, out1


def linear_glu_w4(x, packed, scales, out=None):
    """linear_glu() with the weight as MXFP4 nibbles + block scale bytes."""
    M, N2, K = _w4(x, packed, scales)
    assert N2 % 2 == 0
    if out is None:
        out = torch.empty((M, N2 // 2), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_glu_w4_bf16(ptr(x), _rows(x), ptr(packed), ptr(scales), ptr(out), _rows(out), M, N2 // 2, K, stream_ptr()))
    return out


def repack_int4(layout, qweight, qzeros, scales, G, g_idx=None):
    """One AWQ / GPTQ checkpoint Linear -> the device layout of the grouped int4 weight stream (td_repack_int4), in one launch.
    layout INT4_AWQ: qweight int32 [K, N / 8], qzeros int32 [K / G, N / 8], scales fp16 [K / G, N] (AutoAWQ "GEMM");
    layout INT4_GPTQ (| INT4_GPTQ_V2): qweight int32 [K / 8, N], qzeros int32 [K / G, N / 8], scales fp16 [K / G, N]; g_idx is not read (only k // G is served).
    -> (packed uint8 [N, K / 2], scales fp16 [N, K / G], zeros uint8 [N, K / G]).  The nibble order inside `packed` is the library's own."""
    assert qweight.dtype == torch.int32 and qzeros.dtype == torch.int32 and scales.dtype == torch.float16, (qweight.dtype, qzeros.dtype, scales.dtype)
    assert qweight.dim() == 2 and qweight.is_contiguous() and qzeros.is_contiguous() and scales.is_contiguous()
    if layout == INT4_AWQ:
        K, N = qweight.shape[0], qweight.shape[1] * 8
    else:
        K, N = qweight.shape[0] * 8, qweight.shape[1]
    assert G in INT4_GROUP_SIZES and K % G == 0, (K, G)
    assert qzeros.shape == (K // G, N // 8) and scales.shape == (K // G, N), (qzeros.shape, scales.shape, N, K, G)
    dev = qweight.device
    packed = torch.empty((N, K // 2), dtype=torch.uint8, device=dev)
    s_out = torch.empty((N, K // G), dtype=torch.float16, device=dev)
    z_out = torch.empty((N, K // G), dtype=torch.uint8, device=dev)
    check(lib().td_repack_int4(layout, ptr(qweight), ptr(qzeros), ptr(scales), ptr(g_idx), N, K, G, ptr(packed), ptr(s_out), ptr(z_out), stream_ptr()))
    return packed, s_out, z_out


def _i4(x, packed, scales, zeros, G):
    M, K = x.shape
    N = packed.shape[0]
    assert packed.dtype == torch.uint8 and packed.dim() == 2 and packed.is_contiguous() and packed.shape[1] * 2 == K, (packed.shape, packed.dtype, K)
    assert scales.dtype == torch.float16 and scales.is_contiguous() and scales.shape == (N, K // G), (scales.shape, scales.dtype, K, G)
    assert zeros.dtype == torch.uint8 and zeros.is_contiguous() and zeros.shape == (N, K // G), (zeros.shape, zeros.dtype, K, G)
    return M, N, K


def dequant_rows_int4(packed, scales, zeros, G, out=None):
    """packed [N, K / 2] + scales fp16 [N, K / G] + zeros uint8 [N, K / G] -> bf16 [N, K] = bf16_rne((q - z) s): one rounding (td_dequant_rows_int4)."""
    assert packed.dtype == torch.uint8 and packed.dim() == 2 and packed.is_contiguous()
    N, K = packed.shape[0], packed.shape[1] * 2
    assert scales.dtype == torch.float16 and zeros.dtype == torch.uint8 and scales.is_contiguous() and zeros.is_contiguous()
    assert scales.shape == (N, K // G) and zeros.shape == (N, K // G), (scales.shape, zeros.shape, N, K, G)
    if out is None:
        out = torch.empty((N, K), dtype=torch.bfloat16, device=packed.device)
    assert out.dtype == torch.bfloat16 and out.stride(1) == 1
    check(lib().td_dequant_rows_int4(ptr(packed), ptr(scales), ptr(zeros), G, ptr(out), out.stride(0), N, K, stream_ptr()))
    return out


def linear_i4(x, packed, scales, zeros, G, bias=None, act=ACT_NONE, gate=None, res=None, out=None):
    """linear() with the weight as grouped int4 nibbles + fp16 group scales + zero points (the AWQ / GPTQ weight stream; M <= 64)."""
    M, N, K = _i4(x, packed, scales, zeros, G)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_i4_bf16(ptr(x), _rows(x), ptr(packed), ptr(scales), ptr(zeros), G, ptr(bias), ptr(out), _rows(out), M, N, K, act,
                                  ptr(gate), ptr(res), _rows(res) if res is not None else 0, stream_ptr()))
    return out


def linear_split_i4(x, packed, scales, zeros, G, bias, out0, act0, out1, act1, n_split):
    M, N, K = _i4(x, packed, scales, zeros, G)
    check(lib().td_linear_split_i4_bf16(ptr(x), _rows(x), ptr(packed), ptr(scales), ptr(zeros), G, ptr(bias), ptr(out0), _rows(out0), act0,
                                        ptr(out1), _rows(out1), act1, M, N, K, n_split, stream_ptr()))
    return out0, out1


def linear_glu_i4(x, packed, scales, zeros, G, out=None):
    """linear_glu() with the weight as grouped int4 nibbles + fp16 group scales + zero points."""
    M, N2, K = _i4(x, packed, scales, zeros, G)
    assert N2 % 2 == 0
    if out is None:
        out = torch.empty((M, N2 // 2), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_glu_i4_bf16(ptr(x), _rows(x), ptr(packed), ptr(scales), ptr(zeros), G, ptr(out), _rows(out), M, N2 // 2, K, stream_ptr()))
    return out


def linear_glu(x, w, out=None):
    """out[m, n] = bf16(bf16(silu(bf16(x . w[n]))) * bf16(x . w[I + n])) for w = [gate rows | up rows] ([2 I, K]); M <= 64 (td_linear_glu_bf16)."""
    M, K = x.shape
    assert w.dim() == 2 and w.is_contiguous() and w.shape[1] == K and w.shape[0] % 2 == 0
    inter = w.shape[0] // 2
    if out is None:
        out = torch.empty((M, inter), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_glu_bf16(ptr(x), _rows(x), ptr(w), ptr(out), _rows(out), M, inter, K, stream_ptr()))
    return out


def linear_glu_w8(x, wq, w_scale, out=None):
    """linear_glu() with the weight as e4m3 bytes + row scales."""
    M, N2, K = _w8(x, wq, w_scale)
    assert N2 % 2 == 0
    if out is None:
        out = torch.empty((M, N2 // 2), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_glu_w8_bf16(ptr(x), _rows(x), ptr(wq), ptr(w_scale), ptr(out), _rows(out), M, N2 // 2, K, stream_ptr()))
    return out


def linear_splitk(x, w, bias=None, res=None, out=None, out1=None, n_split=0, split_k=-1, tile_cfg=-1, norm_w=None, norm_out=None, norm_eps=1e-6):
    """out = x @ w.T + bias + res with the contraction split over workgroups (td_linear_splitk_bf16); columns >= n_split go to out1 when given;
    norm_w / norm_out: the reduction also writes RMSNorm(out; norm_w)."""
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous()
    if out is None:
        out = torch.empty((M, n_split if out1 is not None else N), dtype=torch.bfloat16, device=x.device)
    check(lib().td_linear_splitk_bf16(ptr(x), _rows(x), ptr(w), ptr(bias), ptr(out), _rows(out), ptr(out1), _rows(out1) if out1 is not None else 0, n_split,
                                      M, N, K, ptr(res), _rows(res) if res is not None else 0, tile_cfg, split_k,
                                      ptr(norm_w), ptr(norm_out), _rows(norm_out) if norm_out is not None else 0, norm_eps, stream_ptr()))
    return out


def linear_split(x, w, bias, out0, act0, out1, act1, n_split):
    M, K = x.shape
    N = w.shape[0]
    check(lib().td_linear_split_bf16(ptr(x), _rows(x), ptr(w), ptr(bias), ptr(out0), _rows(out0), act0,
                                     ptr(out1), _rows(out1), act1, M, N, K, n_split, stream_ptr()))
    return out0, out1


def attention(q, k, v, out, Hq, Hkv, scale=None, causal=False):
    """q:[B,Sq,>=Hq*128] k,v:[B,Skv,>=Hkv*128] (views into projection outputs) -> out:[B,Sq,>=Hq*128]."""
    assert q.dim() == 3 and k.dim() == 3 and v.dim() == 3 and out.dim() == 3
    B, Sq, _ = q.shape
    Skv = k.shape[1]
    for t in (q, k, v, out):
        assert t.dtype == torch.bfloat16 and t.stride(2) == 1
    assert k.stride() == v.stride()
    if scale is None:
        scale = 128 ** -0.5
    check(lib().td_attention_bf16(ptr(q), q.stride(1), q.stride(0), ptr(k), ptr(v), k.stride(1), k.stride(0),
                                  ptr(out), out.stride(1), out.stride(0), B, Sq, Skv, Hq, Hkv, 128,
                                  float(scale), int(causal), stream_ptr()))
    return out


def attention_joint_prescaled(q, k, v, out, H, score_bound=0.0):
    """The FLUX engine's form of the joint attention: q [S, >= H*128] already multiplied by scale * log2(e); `score_bound` > 0 = a fixed
    reference point of the softmax (td_attention_joint_prescaled_bf16)."""
    for t in (q, k, v, out):
        assert t.dim() == 2 and t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert k.stride() == v.stride() and q.shape[0] == k.shape[0]
    check(lib().td_attention_joint_prescaled_bf16(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(out), out.stride(0), q.shape[0], H, float(score_bound), stream_ptr()))
    return out


def attention_fp8(q, k, v, out, H, scale=None, workspace=None):
    """Joint attention on the e4m3 MFMA: q, k, v, out [S, >= H*128] bf16 views (one batch entry); returns out.
    `workspace`: optional uint8 tensor of td_attention_fp8_workspace_bytes (tests read the packed operands back from it)."""
    assert q.dim() == 2 and k.dim() == 2 and v.dim() == 2 and out.dim() == 2
    for t in (q, k, v, out):
        assert t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert k.stride() == v.stride()
    Sq, Skv = q.shape[0], k.shape[0]
    if scale is None:
        scale = 128 ** -0.5
    L = lib()
    nbytes = int(L.td_attention_fp8_workspace_bytes(Sq, Skv, H))
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_contiguous()
    check(L.td_attention_fp8(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(out), out.stride(0), Sq, Skv, H,
                             float(scale), ptr(ws), stream_ptr()))
    return out


def attention_fp8_qk_rope(qkv, out, H, cos, sin, split=0, wqA=None, wkA=None, wqB=None, wkB=None, eps=1e-6, scale=None, workspace=None):
    """td_attention_fp8 fed from the RAW fused projection qkv [S, 3*H*128] (q | k | v): QK-RMSNorm + RoPE happen inside the pack
    pass (td_attention_fp8_qk_rope); qkv is not modified.  Returns out."""
    assert qkv.dim() == 2 and qkv.dtype == torch.bfloat16 and qkv.stride(1) == 1 and out.dtype == torch.bfloat16 and out.stride(1) == 1
    S, D = qkv.shape[0], H * 128
    assert qkv.shape[1] >= 3 * D and cos.dtype == torch.float32 and cos.shape == (S, 128) and sin.shape == (S, 128)
    if scale is None:
        scale = 128 ** -0.5
    L = lib()
    nbytes = int(L.td_attention_fp8_workspace_bytes(S, S, H))
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes and ws.is_contiguous()
    check(L.td_attention_fp8_qk_rope(ptr(qkv), qkv.stride(0), 0, D, 2 * D, ptr(out), out.stride(0), S, H, ptr(cos), ptr(sin), split,
                                     ptr(wqA), ptr(wkA), ptr(wqB), ptr(wkB), float(eps), float(scale), ptr(ws), stream_ptr()))
    return out


class TdFluxConfig(ctypes.Structure):
    """Mirror of `struct TdFluxConfig` (include/thinkdiff_hip.h)."""
    _fields_ = [("in_channels", ctypes.c_int), ("num_layers", ctypes.c_int), ("num_single_layers", ctypes.c_int),
                ("num_heads", ctypes.c_int), ("head_dim", ctypes.c_int), ("joint_dim", ctypes.c_int),
                ("pooled_dim", ctypes.c_int), ("guidance_embeds", ctypes.c_int), ("mlp_ratio", ctypes.c_int),
                ("axes_dims", ctypes.c_int * 3), ("rope_theta", ctypes.c_float), ("out_channels", ctypes.c_int)]


def norm_rows(x, out=None, rms=False, eps=1e-6, w=None, split=0, shiftA=None, scaleA=None, shiftB=None, scaleB=None):
    rows, D = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib().td_norm_rows_bf16(ptr(x), _rows(x), ptr(out), _rows(out), rows, D, int(rms), float(eps), ptr(w), split,
                                  ptr(shiftA), ptr(scaleA), ptr(shiftB), ptr(scaleB), stream_ptr()))
    return out


def qk_norm_rope(qkv, Hq, Hk, q_col, k_col, cos, sin, split=0, wqA=None, wkA=None, wqB=None, wkB=None, eps=1e-6,
                 rotate_half=False):
    assert cos.dtype == torch.float32 and cos.shape == (qkv.shape[0], 128) and cos.is_contiguous() and sin.is_contiguous()
    check(lib().td_qk_norm_rope_bf16(ptr(qkv), _rows(qkv), qkv.shape[0], Hq, Hk, q_col, k_col, ptr(cos), ptr(sin), split,
                                     ptr(wqA), ptr(wkA), ptr(wqB if wqB is not None else wqA),
                                     ptr(wkB if wkB is not None else wkA), float(eps), int(rotate_half), stream_ptr()))
    return qkv


def qk_norm_rope_premul(qkv, Hq, Hk, q_col, k_col, cos, sin, split=0, wqA=None, wkA=None, wqB=None, wkB=None, eps=1e-6,
                        rotate_half=False, q_premul=1.0):
    """td_qk_norm_rope_premul_bf16: qk_norm_rope with q (not k) multiplied by q_premul in front of its one bf16 rounding, as the FLUX engine runs it."""
    assert cos.dtype == torch.float32 and cos.shape == (qkv.shape[0], 128) and cos.is_contiguous() and sin.is_contiguous()
    check(lib().td_qk_norm_rope_premul_bf16(ptr(qkv), _rows(qkv), qkv.shape[0], Hq, Hk, q_col, k_col, ptr(cos), ptr(sin), split,
                                            ptr(wqA), ptr(wkA), ptr(wqB if wqB is not None else wqA),
                                            ptr(wkB if wkB is not None else wkA), float(eps), int(rotate_half), float(q_premul), stream_ptr()))
    return qkv


def temb_combine_silu(te, ge, pe, want_temb=True):
    """td_temb_combine_silu_bf16: te bf16 [n, D], ge bf16 [D] or None, pe bf16 [D] -> (temb or None, silu(temb)), both bf16 [n, D]."""
    assert te.dim() == 2 and te.is_contiguous() and te.dtype == torch.bfloat16
    n, D = te.shape
    for t in (ge, pe):
        assert t is None or (t.dtype == torch.bfloat16 and t.shape == (D,) and t.is_contiguous())
    temb = torch.empty_like(te) if want_temb else None
    silu_out = torch.empty_like(te)
    check(lib().td_temb_combine_silu_bf16(ptr(te), ptr(ge), ptr(pe), n, D, ptr(temb), ptr(silu_out), stream_ptr()))
    return temb, silu_out


def copy_cols(src, dst, cols):
    """td_copy_cols_bf16: dst[:, :cols] = src[:, :cols] for two bf16 matrices of the same row count (row strides may exceed the widths)."""
    assert src.shape[0] == dst.shape[0]
    check(lib().td_copy_cols_bf16(ptr(src), _rows(src), ptr(dst), _rows(dst), src.shape[0], cols, stream_ptr()))
    return dst


def flux_rope_table(ids, axes_dims=(16, 56, 56), theta=10000.0):
    assert ids.dtype == torch.float32 and ids.is_contiguous() and ids.shape[1] == 3
    S = ids.shape[0]
    cos = torch.empty(S, 128, dtype=torch.float32, device=ids.device)
    sin = torch.empty_like(cos)
    axes = (ctypes.c_int * 3)(*axes_dims)
    check(lib().td_flux_rope_table(ptr(ids), S, ctypes.cast(axes, ctypes.c_void_p), float(theta), ptr(cos), ptr(sin), stream_ptr()))
    return cos, sin


def mrope_table(pos, sections=(16, 24, 24), theta=1e6, round_bf16=True):
    """td_mrope_table: pos int32 [3, n] (temporal, height, width) -> cos, sin fp32 [n, 128]."""
    assert pos.dtype == torch.int32 and pos.dim() == 2 and pos.shape[0] == 3 and pos.is_contiguous()
    n = pos.shape[1]
    cos = torch.empty(n, 128, dtype=torch.float32, device=pos.device)
    sin = torch.empty_like(cos)
    sec = (ctypes.c_int * 3)(*sections)
    check(lib().td_mrope_table(ptr(pos), n, ctypes.cast(sec, ctypes.c_void_p), float(theta), int(round_bf16), ptr(cos), ptr(sin), stream_ptr()))
    return cos, sin


def embed_gather(ids, table, out=None):
    """td_embed_gather_bf16: out[i, :] = table[ids[i], :]; ids int32 [n] on the device, table bf16 [vocab, D].  Ids outside [0, vocab) are clamped."""
    assert ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous()
    assert table.dtype == torch.bfloat16 and table.dim() == 2 and table.is_contiguous()
    n, (vocab, D) = ids.numel(), table.shape
    if out is None:
        out = torch.empty(n, D, dtype=torch.bfloat16, device=table.device)
    assert out.shape == (n, D) and out.is_contiguous() and out.dtype == torch.bfloat16
    check(lib().td_embed_gather_bf16(ptr(ids), ptr(table), ptr(out), n, D, vocab, stream_ptr()))
    return out


def timestep_sincos(t):
    assert t.dtype == torch.float32 and t.is_contiguous()
    out = torch.empty(t.numel(), 256, dtype=torch.bfloat16, device=t.device)
    check(lib().td_timestep_sincos(ptr(t), t.numel(), ptr(out), stream_ptr()))
    return out


def euler_step(x, v, dt):
    assert x.is_contiguous() and v.is_contiguous() and x.dtype == v.dtype == torch.bfloat16
    check(lib().td_euler_step_bf16(ptr(x), ptr(v), float(dt), x.numel(), stream_ptr()))
    return x


def flux_pack_latents(lat):
    """[C,H,W] bf16 -> [(H/2)(W/2), 4C]"""
    C, H, W = lat.shape
    out = torch.empty((H // 2) * (W // 2), C * 4, dtype=torch.bfloat16, device=lat.device)
    check(lib().td_flux_pack_latents(ptr(lat.contiguous()), ptr(out), C, H, W, 0, 1.0, 0.0, stream_ptr()))
    return out


def flux_unpack_latents(x, C, H, W, div=1.0, add=0.0):
    """[(H/2)(W/2), 4C] bf16 -> bf16(bf16([C,H,W] / div) + add)"""
    out = torch.empty(C, H, W, dtype=torch.bfloat16, device=x.device)
    check(lib().td_flux_pack_latents(ptr(x.contiguous()), ptr(out), C, H, W, 1, float(div), float(add), stream_ptr()))
    return out


def cls_avgpool2(x):
    n, C = x.shape
    G = int(round((n - 1) ** 0.5))
    assert G * G == n - 1 and x.is_contiguous()
    out = torch.empty(1 + (G // 2) ** 2, C, dtype=torch.bfloat16, device=x.device)
    check(lib().td_cls_avgpool2_bf16(ptr(x), ptr(out), G, C, stream_ptr()))
    return out


def fill_normal(t, seed, std=1.0, mean=0.0):
    assert t.is_contiguous() and t.dtype == torch.bfloat16
    check(lib().td_fill_normal_bf16(ptr(t), t.numel(), seed, float(std), float(mean), stream_ptr()))
    return t


def fill_normal_from(t, seed, pair0, std=1.0, mean=0.0):
    """td_fill_normal_from_bf16: t is a piece of a larger buffer; element i draws what element 2 * pair0 + i of fill_normal with this seed draws."""
    assert t.is_contiguous() and t.dtype == torch.bfloat16
    check(lib().td_fill_normal_from_bf16(ptr(t), t.numel(), seed, float(std), float(mean), int(pair0), stream_ptr()))
    return t


def aligner_mlp2x(x, w0, b0, w2, b2, norm_w, eps=1e-6, fp32_norm=False):
    """y = T5LayerNorm(Linear2(GELU(Linear0(x))))  x:[M,K] bf16 -> [M,hidden] bf16"""
    M, K = x.shape
    hidden = w0.shape[0]
    ws = torch.empty(2 * M * hidden, dtype=torch.bfloat16, device=x.device)
    y = torch.empty(M, hidden, dtype=torch.bfloat16, device=x.device)
    check(lib().td_aligner_mlp2x_bf16(ptr(x), _rows(x), M, K, hidden, ptr(w0), ptr(b0), ptr(w2), ptr(b2), ptr(norm_w),
                                      float(eps), int(fp32_norm), ptr(ws), ptr(y), hidden, stream_ptr()))
    return y


def linear_grouped2(x0, w0, b0, y0, x1, w1, b1, y1, act=ACT_NONE, gate0=None, res0=None, gate1=None, res1=None, tile_cfg=-1):
    """Two Linear problems (same N, K, row strides) in one launch; x1 may be None (M1 = 0)."""
    M0, K = x0.shape
    N = w0.shape[0]
    M1 = 0 if x1 is None else x1.shape[0]
    ldr = _rows(res0) if res0 is not None else 0
    check(lib().td_linear_grouped2_bf16(ptr(x0), M0, ptr(w0), ptr(b0), ptr(gate0), ptr(res0), ptr(y0),
                                        ptr(x1), M1, ptr(w1), ptr(b1), ptr(gate1), ptr(res1), ptr(y1),
                                        _rows(x0), _rows(y0), ldr, N, K, act, tile_cfg, stream_ptr()))
    return y0, y1


OPERAND_BF16, OPERAND_INT8, OPERAND_E4M3 = 0, 1, 2


def gemm_plan(M, N, K, shared=False, operand=OPERAND_BF16):
    """td_gemm_plan_query: the tile an automatic launch of an M x N x K Linear takes (0 256x256, 1 256x64, 2 32x256, 3 288x192), alone on the
    chip or under the shared-chip hint of several images in flight.  Host arithmetic: needs no GPU."""
    cfg = lib().td_gemm_plan_query(int(M), int(N), int(K), int(bool(shared)), int(operand))
    if cfg < 0:
        raise ThinkDiffHipError(lib().td_last_error().decode())
    return cfg


def linear_drain(x0, w0, b0, y0, x1=None, w1=None, b1=None, y1=None, act=ACT_NONE, gate0=None, res0=None, gate1=None, res1=None,
                 y_split=None, act_split=ACT_NONE, n_split=0, max_workgroups=0):
    """td_linear_drain_bf16: linear_grouped2 (or, with y_split, the split-output Linear) on the 256x256 tile with at most max_workgroups
    walking workgroups (0: no bound)."""
    M0, K = x0.shape
    N = w0.shape[0]
    M1 = 0 if x1 is None else x1.shape[0]
    ldr = _rows(res0) if res0 is not None else 0
    check(lib().td_linear_drain_bf16(ptr(x0), M0, ptr(w0), ptr(b0), ptr(gate0), ptr(res0), ptr(y0),
                                     ptr(x1), M1, ptr(w1), ptr(b1), ptr(gate1), ptr(res1), ptr(y1),
                                     _rows(x0), _rows(y0), ldr, N, K, act,
                                     ptr(y_split), _rows(y_split) if y_split is not None else 0, act_split, n_split, max_workgroups, stream_ptr()))
    return y0


class TdQwen2Config(ctypes.Structure):
    """Mirror of `struct TdQwen2Config` (include/thinkdiff_hip.h)."""
    _fields_ = [("hidden", ctypes.c_int), ("num_layers", ctypes.c_int), ("num_heads", ctypes.c_int),
                ("num_kv_heads", ctypes.c_int), ("head_dim", ctypes.c_int), ("intermediate", ctypes.c_int),
                ("vocab", ctypes.c_int), ("tie_embeddings", ctypes.c_int), ("mrope_section", ctypes.c_int * 3),
                ("rms_eps", ctypes.c_float), ("rope_theta", ctypes.c_float)]


class TdKvPlane(ctypes.Structure):
    """Mirror of `struct TdKvPlane` (include/thinkdiff_hip.h): slot s of a cache plane starts at base + s * slot_rows * row_bytes."""
    _fields_ = [("base", ctypes.c_void_p), ("row_bytes", ctypes.c_int64), ("slot_rows", ctypes.c_int64)]


def kv_fork_rows(planes, src_slot, dst_slots, n_rows):
    """td_kv_fork_rows: rows [0, n_rows) of slot src_slot -> the same rows of every slot of dst_slots, for every plane in one launch.
    planes: (tensor, slot_rows) pairs, each tensor a contiguous device array of slots x slot_rows rows (any dtype); in place."""
    arr = (TdKvPlane * max(1, len(planes)))()
    for i, (t, slot_rows) in enumerate(planes):
        if not t.is_contiguous() or t.dim() < 2 or t.shape[0] % int(slot_rows):
            raise ThinkDiffHipError(f"kv_fork_rows: plane {i} must be contiguous [slots * slot_rows, ...] with slot_rows={slot_rows} dividing its {t.shape[0]} rows")
        slots = t.shape[0] // int(slot_rows)
        bad = [int(s) for s in [src_slot, *dst_slots] if not 0 <= int(s) < slots]
        if bad:
            raise ThinkDiffHipError(f"kv_fork_rows: slot {bad[0]} outside the {slots} slots of plane {i}")
        arr[i] = TdKvPlane(t.data_ptr(), (t.numel() // t.shape[0]) * t.element_size(), int(slot_rows))
    dst = (ctypes.c_int * max(1, len(dst_slots)))(*[int(d) for d in dst_slots])
    check(lib().td_kv_fork_rows(ctypes.cast(arr, ctypes.c_void_p), len(planes), int(src_slot), ctypes.cast(dst, ctypes.c_void_p), len(dst_slots), int(n_rows),
                                stream_ptr()))


def kv_gather_rows(planes, slots, copy_src, n_rows):
    """td_kv_gather_rows: for every row j with copy_src[j] >= 0, rows [0, n_rows[j]) of slot slots[copy_src[j]] -> the same rows of slot slots[j], on every
    plane.  planes: (tensor, slot_rows) pairs as for kv_fork_rows; slots / n_rows: host ints, one per row (n_rows may be one int for all);
    copy_src: an int32 DEVICE tensor [len(slots)] (a list is uploaded), read by the kernel.  The caller vouches that no destination slot is a
    source of the same call.  In place."""
    n = len(slots)
    if isinstance(n_rows, int):
        n_rows = [n_rows] * n
    if len(n_rows) != n:
        raise ThinkDiffHipError(f"kv_gather_rows: {len(n_rows)} n_rows for {n} slots")
    arr = (TdKvPlane * max(1, len(planes)))()
    dev = None
    for i, (t, slot_rows) in enumerate(planes):
        if not t.is_contiguous() or t.dim() < 2 or t.shape[0] % int(slot_rows):
            raise ThinkDiffHipError(f"kv_gather_rows: plane {i} must be contiguous [slots * slot_rows, ...] with slot_rows={slot_rows} dividing its {t.shape[0]} rows")
        n_slots = t.shape[0] // int(slot_rows)
        bad = [int(s) for s in slots if not 0 <= int(s) < n_slots]
        if bad:
            raise ThinkDiffHipError(f"kv_gather_rows: slot {bad[0]} outside the {n_slots} slots of plane {i}")
        arr[i] = TdKvPlane(t.data_ptr(), (t.numel() // t.shape[0]) * t.element_size(), int(slot_rows))
        dev = t.device
    if not torch.is_tensor(copy_src):
        copy_src = torch.tensor([int(c) for c in copy_src], dtype=torch.int32)
    copy_src = copy_src.to(device=dev, dtype=torch.int32).contiguous()
    if copy_src.numel() != n:
        raise ThinkDiffHipError(f"kv_gather_rows: {copy_src.numel()} copy_src entries for {n} slots")
    sl = (ctypes.c_int * max(1, n))(*[int(s) for s in slots])
    nr = (ctypes.c_int * max(1, n))(*[int(v) for v in n_rows])
    check(lib().td_kv_gather_rows(ctypes.cast(arr, ctypes.c_void_p), len(planes), n, ctypes.cast(sl, ctypes.c_void_p), ptr(copy_src),
                                  ctypes.cast(nr, ctypes.c_void_p), stream_ptr()))


LORA_ROWS_MAX_ADAPTERS = 8     # TD_LORA_MAX_ADAPTERS
LORA_ROWS_MAX_SEGS = 3         # TD_LORA_ROWS_MAX_SEGS
LORA_ROWS_MAX_RANK = 64        # TD_LORA_ROWS_MAX_RANK


def lora_rows_pack(A, B):
    """td_lora_rows_pack_bf16: the kernels' operand form of one (lora_A.weight [r, K], lora_B.weight [N, r]) bf16 pair: Ap [r_pad, K] then Bp [N, r_pad], the
    rank zero-padded to a multiple of 16.  Returns a uint8 device tensor."""
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and A.dim() == 2 and B.dim() == 2 and A.shape[0] == B.shape[1], (A.shape, B.shape)
    A, B = A.contiguous(), B.contiguous()
    r, K = A.shape
    N = B.shape[0]
    packed = torch.empty(max(16, lib().td_lora_rows_packed_bytes(int(r), int(N), int(K))), dtype=torch.uint8, device=A.device)
    check(lib().td_lora_rows_pack_bf16(ptr(A), ptr(B), int(r), int(N), int(K), ptr(packed), stream_ptr()))
    return packed


def lora_rows_workspace_bytes(rows, K, n_segs, max_rank):
    return int(lib().td_lora_rows_workspace_bytes(int(rows), int(K), int(n_segs), int(max_rank)))


def lora_rows(x, row_adapter, packed, ranks, scales, ys, workspace=None):
    """td_lora_rows_bf16: ys[s][row] += scales[a] * B_as (bf16(A_as x[row])) for a = row_adapter[row] >= 0, in place, one rounding (csrc/lora_rows.hip).
    x bf16 [rows, K] (row stride free); row_adapter int32 device [rows]; packed[a][s]: lora_rows_pack of adapter a's pair for segment s, or None;
    ranks / scales: one per adapter; ys: 1 to 3 bf16 [rows, width_s] views (row stride free), the output segments.  Returns ys."""
    ldx = _rows(x)
    rows, K = x.shape
    n_ad, n_segs = len(packed), len(ys)
    ptrs = (ctypes.c_void_p * max(1, n_ad * n_segs))()
    for a, per in enumerate(packed):
        if len(per) != n_segs:
            raise ThinkDiffHipError(f"lora_rows: adapter {a} gives {len(per)} operands for {n_segs} segments")
        for s, p in enumerate(per):
            ptrs[a * n_segs + s] = None if p is None else p.data_ptr()
    rk = (ctypes.c_int * max(1, n_ad))(*[int(r) for r in ranks])
    sc = (ctypes.c_float * max(1, n_ad))(*[float(v) for v in scales])
    yp = (ctypes.c_void_p * n_segs)(*[y.data_ptr() for y in ys])
    ld = (ctypes.c_int64 * n_segs)(*[_rows(y) for y in ys])
    wd = (ctypes.c_int * n_segs)(*[int(y.shape[1]) for y in ys])
    if any(y.shape[0] != rows for y in ys) or row_adapter.numel() != rows or row_adapter.dtype != torch.int32:
        raise ThinkDiffHipError(f"lora_rows: every output and the int32 row_adapter need {rows} rows")
    if workspace is None:
        max_rank = max([int(r) for r, per in zip(ranks, packed) if any(p is not None for p in per)] or [1])
        workspace = torch.empty(max(16, lora_rows_workspace_bytes(rows, K, n_segs, max_rank)), dtype=torch.uint8, device=x.device)
    check(lib().td_lora_rows_bf16(ptr(x), ldx, int(rows), int(K), ptr(row_adapter), n_ad, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(rk, ctypes.c_void_p),
                                  ctypes.cast(sc, ctypes.c_void_p), n_segs, ctypes.cast(yp, ctypes.c_void_p), ctypes.cast(ld, ctypes.c_void_p),
                                  ctypes.cast(wd, ctypes.c_void_p), ptr(workspace), workspace.numel(), stream_ptr()))
    return ys


MAX_BEAM_WIDTH = 10        # TD_MAX_BEAM_WIDTH (2 W candidates per row must fit TD_MAX_LOGPROBS)


def beam_select(top_ids, top_lp, cum_in, rank_in, W, n_in, eos=-1, out=None):
    """td_beam_select: one beam-search step for R requests of W rows.  top_ids int32 / top_lp fp32 [R*W, cap] (logprobs_rows with n_top = 2W), cum_in
    fp32 [R*W], rank_in int32 [R*W]; n_in = 1 at the first step (only row r*W of a request is live), W afterwards; eos: a token id or -1.
    -> (token, cum_out, rank_out, copy_src, parent, fin_flag, fin_cum), [R*W] device tensors; `out`: that tuple to write into (slices of [T, R*W] logs)."""
    W = int(W)
    if not (top_ids.dim() == 2 and top_ids.dtype == torch.int32 and top_ids.is_contiguous() and top_lp.dtype == torch.float32 and top_lp.is_contiguous()
            and top_lp.shape == top_ids.shape):
        raise ThinkDiffHipError("beam_select: top_ids int32 and top_lp fp32 must be contiguous [R*W, cap] tensors of one shape")
    rows, cap = top_ids.shape
    if W < 1 or rows % W:
        raise ThinkDiffHipError(f"beam_select: W={W} does not divide the {rows} rows")
    dev = top_ids.device
    cum_in = cum_in.to(device=dev, dtype=torch.float32).contiguous()
    rank_in = rank_in.to(device=dev, dtype=torch.int32).contiguous()
    if out is None:
        out = tuple(torch.empty(rows, dtype=torch.float32 if i in (1, 6) else torch.int32, device=dev) for i in range(7))
    for i, t in enumerate((cum_in, rank_in) + tuple(out)):
        want = torch.float32 if i in (0, 3, 8) else torch.int32
        if t.dtype != want or t.numel() != rows or not t.is_contiguous() or t.device != dev:
            raise ThinkDiffHipError(f"beam_select: tensor {i} of (cum_in, rank_in, token, cum_out, rank_out, copy_src, parent, fin_flag, fin_cum) must be a "
                                    f"contiguous {want} tensor of {rows} entries on {dev}")
    check(lib().td_beam_select(ptr(top_ids), ptr(top_lp), int(cap), ptr(cum_in), ptr(rank_in), rows // W, W, int(n_in), int(eos), *[ptr(t) for t in out],
                               stream_ptr()))
    return tuple(out)


MAX_VERIFY_ROWS = 8        # TD_MAX_VERIFY_ROWS


def _seq_ints(t, n, what, dev):
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n or t.device != dev:
        raise ThinkDiffHipError(f"{what} must be a contiguous int32 tensor of {n} entries on {dev}")
    return t


def attention_verify(q, cache, seq_row0, seq_rows, seq_len0, seq_slot, Hq, Hkv, scale=None, out=None, t_max=None, max_len=None):
    """td_attention_verify: multi-row decode attention.  q bf16 [R, >= Hq*128]; `cache` = (k, v) bf16 [slots, S, >= Hkv*128] views of one cache, or
    (k8, v8, k_scale, v_scale) for the e4m3 form (uint8 [slots, S, >= Hkv*128], fp32 [slots, S, >= Hkv]); the four per-sequence int32 device tensors
    [n_seq]: first q row, rows (1..8), keys visible to the first row, cache slot.  -> out bf16 [R, Hq*128]; rows no sequence owns are left alone.
    t_max / max_len: what the host knows of seq_rows' maximum and of the longest visible length (td_attention_verify_ex; None: 8 rows, length unknown)."""
    dev, n = q.device, seq_row0.numel()
    if not (q.dim() == 2 and q.dtype == torch.bfloat16 and q.stride(1) == 1):
        raise ThinkDiffHipError("attention_verify: q must be a bf16 [R, Hq*128] tensor with unit column stride")
    for name, t in (("seq_row0", seq_row0), ("seq_rows", seq_rows), ("seq_len0", seq_len0), ("seq_slot", seq_slot)):
        _seq_ints(t, n, f"attention_verify: {name}", dev)
    if len(cache) not in (2, 4):
        raise ThinkDiffHipError(f"attention_verify: cache holds {len(cache)} tensors: (k, v) or (k8, v8, k_scale, v_scale)")
    k, v = cache[0], cache[1]
    want = torch.bfloat16 if len(cache) == 2 else torch.uint8
    if not (k.dim() == 3 and k.dtype == want and v.dtype == want and k.stride(2) == 1 and k.stride() == v.stride() and k.shape == v.shape):
        raise ThinkDiffHipError(f"attention_verify: the k and v planes must be {want} [slots, S, Hkv*128] views that share shape and strides")
    if out is None:
        out = torch.empty((q.shape[0], Hq * 128), dtype=torch.bfloat16, device=dev)
    if scale is None:
        scale = 128 ** -0.5
    if len(cache) == 2:
        args = (ptr(k), ptr(v), k.stride(1), k.stride(0), None, None, None, None, 0, 0)
    else:
        ks, vs = cache[2], cache[3]
        if not (ks.dim() == 3 and ks.dtype == torch.float32 and vs.dtype == torch.float32 and ks.stride(2) == 1 and ks.stride() == vs.stride()):
            raise ThinkDiffHipError("attention_verify: k_scale and v_scale must be fp32 [slots, S, Hkv] views that share their strides")
        args = (None, None, k.stride(1), k.stride(0), ptr(k), ptr(v), ptr(ks), ptr(vs), ks.stride(1), ks.stride(0))
    check(lib().td_attention_verify_ex(ptr(q), q.stride(0), *args, ptr(out), out.stride(0), n, ptr(seq_row0), ptr(seq_rows), ptr(seq_len0), ptr(seq_slot),
                                       int(Hq), int(Hkv), float(scale), MAX_VERIFY_ROWS if t_max is None else int(t_max), 0 if max_len is None else int(max_len),
                                       stream_ptr()))
    return out


def spec_accept(sampled, fed, seq_row0, seq_rows, out=None):
    """td_spec_accept: sampled / fed int32 [R] (the token sampled from each row's logits, the token fed as that row), seq_row0 / seq_rows int32 [B]
    -> (n_emit int32 [B], emit int32 [B, 8]): per sequence the sampled tokens up to and including the first whose guess behind it was wrong; -1 beyond."""
    dev, B = sampled.device, seq_row0.numel()
    _seq_ints(sampled, sampled.numel(), "spec_accept: sampled", dev)
    _seq_ints(fed, sampled.numel(), "spec_accept: fed", dev)
    _seq_ints(seq_row0, B, "spec_accept: seq_row0", dev)
    _seq_ints(seq_rows, B, "spec_accept: seq_rows", dev)
    if out is None:
        out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, MAX_VERIFY_ROWS, dtype=torch.int32, device=dev))
    _seq_ints(out[0], B, "spec_accept: n_emit", dev)
    _seq_ints(out[1], B * MAX_VERIFY_ROWS, "spec_accept: emit", dev)
    check(lib().td_spec_accept(ptr(sampled), ptr(fed), ptr(seq_row0), ptr(seq_rows), B, ptr(out[0]), ptr(out[1]), stream_ptr()))
    return out


class TdVaeConfig(ctypes.Structure):
    """Mirror of `struct TdVaeConfig` (include/thinkdiff_hip.h)."""
    _fields_ = [("latent_channels", ctypes.c_int), ("out_channels", ctypes.c_int), ("num_blocks", ctypes.c_int),
                ("block_out_channels", ctypes.c_int * 4), ("layers_per_block", ctypes.c_int), ("norm_groups", ctypes.c_int)]


def conv3x3_nhwc(x, w_packed, bias, H, W, Cout, res=None, upsample2x=False, out=None):
    """x [Hin*Win, Cin] bf16 NHWC, w_packed [Cout, 9*Cin] -> [H*W, Cout].  out: the output buffer, which may be `res` itself (the VAE's
    resnet adds its input in place)."""
    Cin = x.shape[1]
    if out is None:
        y = torch.empty(H * W, Cout, dtype=torch.bfloat16, device=x.device)
    else:
        assert out.shape == (H * W, Cout) and out.dtype == torch.bfloat16 and out.is_contiguous() and out.device == x.device
        y = out
    check(lib().td_conv3x3_nhwc_bf16(ptr(x), ptr(w_packed), ptr(bias), ptr(res), ptr(y), H, W, Cin, Cout, int(upsample2x), stream_ptr()))
    return y


def conv3x3_s2_nhwc(x, w_packed, bias, Hin, Win, Cout):
    """Downsample2D's conv: x [Hin*Win, Cin] bf16 NHWC, pad (0,1,0,1), 3x3 stride 2 -> [(Hin/2)(Win/2), Cout]"""
    Cin = x.shape[1]
    y = torch.empty((Hin // 2) * (Win // 2), Cout, dtype=torch.bfloat16, device=x.device)
    check(lib().td_conv3x3_s2_nhwc_bf16(ptr(x), ptr(w_packed), ptr(bias), ptr(y), Hin, Win, Cin, Cout, stream_ptr()))
    return y


IMAGE_U8_HWC, IMAGE_F32_CHW = 0, 1      # TD_IMAGE_* (include/thinkdiff_hip.h)


MASK_U8_HW, MASK_F32_HW = 0, 1          # TD_INPAINT_MASK_* (include/thinkdiff_hip.h)


def vae_image_to_nhwc(image, Cpad=64, mask=None):
    """VaeImageProcessor.preprocess + .to(bf16): uint8 [H, W, 3] or float32 [3, H, W] in [0,1] -> bf16 [H*W, Cpad] (channels >= 3 zero).
    mask (uint8 or float32 [H, W]): FLUX.1 Fill's masked image, image * (1 - binarize(mask)) in fp32 before the cast."""
    u8 = image.dtype == torch.uint8
    H, W = (image.shape[0], image.shape[1]) if u8 else (image.shape[1], image.shape[2])
    out = torch.empty(H * W, Cpad, dtype=torch.bfloat16, device=image.device)
    fmt = IMAGE_U8_HWC if u8 else IMAGE_F32_CHW
    if mask is None:
        check(lib().td_vae_image_to_nhwc_bf16(ptr(image.contiguous()), fmt, H, W, ptr(out), Cpad, stream_ptr()))
    else:
        assert mask.shape == (H, W) and mask.dtype in (torch.uint8, torch.float32) and mask.is_contiguous()
        mfmt = MASK_U8_HW if mask.dtype == torch.uint8 else MASK_F32_HW
        check(lib().td_vae_image_to_nhwc_masked_bf16(ptr(image.contiguous()), fmt, ptr(mask), mfmt, H, W, ptr(out), Cpad, stream_ptr()))
    return out


def conv3x3_pack_weight(w_oihw, Cout_pad=None, Cin_pad=None):
    Cout, Cin = w_oihw.shape[:2]
    Cout_pad, Cin_pad = Cout_pad or Cout, Cin_pad or Cin
    out = torch.empty(Cout_pad, 9 * Cin_pad, dtype=torch.bfloat16, device=w_oihw.device)
    check(lib().td_conv3x3_pack_weight(ptr(w_oihw.contiguous()), ptr(out), Cout, Cin, Cout_pad, Cin_pad, stream_ptr()))
    return out


def vae_latents_to_nhwc(packed, h, w, Cpad, scaling_factor, shift_factor):
    """The first launch of td_vae_decode alone: packed FLUX latents [(h/2)(w/2), 4C] bf16 -> NHWC [h*w, Cpad] bf16,
    `(unpack_latents(packed) / scaling_factor) + shift_factor` with the bf16 rounding points of the torch statement; channels >= C zero."""
    assert packed.dtype == torch.bfloat16 and packed.is_contiguous() and packed.shape[0] == (h // 2) * (w // 2) and packed.shape[1] % 4 == 0
    C = packed.shape[1] // 4
    out = torch.empty(h * w, Cpad, dtype=torch.bfloat16, device=packed.device)
    check(lib().td_vae_latents_to_nhwc_bf16(ptr(packed), ptr(out), C, h, w, Cpad, float(scaling_factor), float(shift_factor), stream_ptr()))
    return out


def vae_image_finalize(x, u8=True, chw=True):
    """The last launch of td_vae_decode alone: x [P, Cpad] bf16 NHWC (three live channels) -> (uint8 [P, 3] or None, bf16 [3, P] or None)."""
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 2
    P, Cpad = x.shape
    o8 = torch.empty(P, 3, dtype=torch.uint8, device=x.device) if u8 else None
    oc = torch.empty(3, P, dtype=torch.bfloat16, device=x.device) if chw else None
    check(lib().td_vae_image_finalize(ptr(x), P, Cpad, ptr(o8), ptr(oc), stream_ptr()))
    return o8, oc


def groupnorm_nhwc(x, gamma, beta, groups=32, eps=1e-6, silu=False):
    P, C = x.shape
    ws = torch.empty(lib().td_groupnorm_workspace_floats(), dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    check(lib().td_groupnorm_nhwc_bf16(ptr(x), ptr(y), P, C, groups, float(eps), ptr(gamma), ptr(beta), int(silu), ptr(ws), stream_ptr()))
    return y


def layernorm(x, w=None, b=None, eps=1e-5, rms=False, out=None):
    rows, D = x.shape
    if out is None:
        out = torch.empty(rows, D, dtype=torch.bfloat16, device=x.device)
    check(lib().td_layernorm_bf16(ptr(x), _rows(x), ptr(out), _rows(out), rows, D, int(rms), float(eps), ptr(w), ptr(b), stream_ptr()))
    return out


def add_rows(a, b):
    rows, D = a.shape
    out = torch.empty_like(a)
    check(lib().td_add_rows_bf16(ptr(a), ptr(b.contiguous()), ptr(out), rows, D, b.shape[0], stream_ptr()))
    return out


def glu_mul(gate_up, act):
    rows, two_i = gate_up.shape
    out = torch.empty(rows, two_i // 2, dtype=torch.bfloat16, device=gate_up.device)
    check(lib().td_glu_mul_bf16(ptr(gate_up), ptr(out), rows, two_i // 2, act, stream_ptr()))
    return out


def attention_padded(qkv, H, scale, causal=False, bias=None, out=None):
    """qkv [S, 3*H*128] with every head zero-padded to 128 columns -> [S, H*128].  bias: fp32 [H,S,S] or None."""
    S = qkv.shape[0]
    W = H * 128
    if out is None:
        out = torch.empty(S, W, dtype=torch.bfloat16, device=qkv.device)
    assert out.shape == (S, W) and out.is_contiguous()
    check(lib().td_attention_bias_bf16(ptr(qkv), _rows(qkv), ptr(qkv[:, W:]), ptr(qkv[:, 2 * W:]), _rows(qkv), ptr(out), W,
                                       S, S, H, H, float(scale), int(causal), ptr(bias), stream_ptr()))
    return out


def attention_bias(q, k, v, out, Hq, Hkv, scale, causal, bias):
    """td_attention_bias_bf16 on separate operand views: q [Sq, >= Hq*128], k, v [Skv, >= Hkv*128] (one row stride for both), out
    [Sq, >= Hq*128], each with its own row stride; bias fp32 [Hq, Sq, Skv] (16-byte aligned, Skv % 4 == 0) or None.
    softmax(q.k^T * scale + bias [+ causal mask: query i sees keys j <= i + Skv - Sq]) . v -> out."""
    for t in (q, k, v, out):
        assert t.dim() == 2 and t.dtype == torch.bfloat16 and t.stride(1) == 1
    Sq, Skv = q.shape[0], k.shape[0]
    assert k.stride() == v.stride() and v.shape[0] == Skv and out.shape[0] == Sq
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.shape == (Hq, Sq, Skv) and bias.is_contiguous()
    check(lib().td_attention_bias_bf16(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(out), out.stride(0),
                                       Sq, Skv, Hq, Hkv, float(scale), int(causal), ptr(bias), stream_ptr()))
    return out


def attention_padded_varlen(qkv, H, scale, seg_starts, max_len, out=None):
    """attention_padded over packed segments in ONE launch: qkv [S, 3*H*128], seg_starts device int32 [n_seg + 1] (row offsets,
    seg_starts[-1] == S), full attention inside each segment.  max_len = the longest segment."""
    S = qkv.shape[0]
    W = H * 128
    if out is None:
        out = torch.empty(S, W, dtype=torch.bfloat16, device=qkv.device)
    assert out.shape == (S, W) and out.is_contiguous()
    assert seg_starts.dtype == torch.int32 and seg_starts.is_cuda and seg_starts.is_contiguous() and seg_starts.numel() >= 2
    check(lib().td_attention_varlen_bf16(ptr(qkv), _rows(qkv), ptr(qkv[:, W:]), ptr(qkv[:, 2 * W:]), _rows(qkv), ptr(out), W,
                                         ptr(seg_starts), seg_starts.numel() - 1, int(max_len), H, H, float(scale), stream_ptr()))
    return out


def attention_segments(q, k, v, out, Hq, Hkv, seg_starts, max_len, scale=None, causal=False):
    """td_attention_segments_bf16 on separate operand views: q, out [S, >= Hq*128], k, v [S, >= Hkv*128] (one row stride for both), each with its own
    row stride; seg_starts device int32 [n_seg + 1] (row offsets, seg_starts[-1] == S); max_len >= the longest segment.  causal: row i of a segment
    sees the segment's rows j <= i (the Qwen2-VL engine's packed prefill launch); otherwise full attention inside each segment."""
    for t in (q, k, v, out):
        assert t.dim() == 2 and t.dtype == torch.bfloat16 and t.stride(1) == 1
    S = q.shape[0]
    assert k.stride() == v.stride() and k.shape[0] == S and v.shape[0] == S and out.shape[0] == S
    assert seg_starts.dtype == torch.int32 and seg_starts.is_cuda and seg_starts.is_contiguous() and seg_starts.numel() >= 2
    if scale is None:
        scale = 128 ** -0.5
    check(lib().td_attention_segments_bf16(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(out), out.stride(0), ptr(seg_starts),
                                           seg_starts.numel() - 1, int(max_len), Hq, Hkv, float(scale), int(causal), stream_ptr()))
    return out


def attention_prefix_segments(q, k, v, out, Hq, Hkv, seg_starts, kv_row0, kv_lens, max_q_len, max_kv_len, scale=None):
    """td_attention_prefix_segments_bf16 (context attention): packed causal query segments q, out [R, >= Hq*128] over key ranges of their own in k, v
    [rows, >= Hkv*128] (one row stride for both: a KV cache seen as rows).  Segment b = q rows [seg_starts[b], seg_starts[b+1]) against key rows
    [kv_row0[b], kv_row0[b] + kv_lens[b]); its last rows are the segment's own tokens, the ones in front its cached prefix.  seg_starts device int32
    [n + 1], kv_row0 / kv_lens device int32 [n]; max_q_len / max_kv_len >= the longest query segment / key range."""
    for t in (q, k, v, out):
        assert t.dim() == 2 and t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert k.stride() == v.stride() and k.shape[0] == v.shape[0] and out.shape[0] == q.shape[0]
    for t in (seg_starts, kv_row0, kv_lens):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    n = kv_row0.numel()
    assert n >= 1 and kv_lens.numel() == n and seg_starts.numel() == n + 1
    if scale is None:
        scale = 128 ** -0.5
    check(lib().td_attention_prefix_segments_bf16(ptr(q), ptr(k), ptr(v), ptr(out), q.stride(0), k.stride(0), out.stride(0), ptr(seg_starts), ptr(kv_row0),
                                                  ptr(kv_lens), n, int(max_q_len), int(max_kv_len), Hq, Hkv, float(scale), stream_ptr()))
    return out


def rope_half(x, H, hd, cos, sin, head_stride=128):
    """In place on x [S, >= H*head_stride]; cos/sin fp32 [S, hd/2]."""
    assert cos.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous() and cos.shape == (x.shape[0], hd // 2)
    check(lib().td_rope_half_bf16(ptr(x), _rows(x), x.shape[0], H, head_stride, hd, ptr(cos), ptr(sin), stream_ptr()))
    return x


def qwen2_patchify_u8(img, lut, patch, merge, temporal, Kpad, out=None):
    """img uint8 [H,W,3] (cuda), lut fp32 [3,256] (cuda) -> bf16 [(H/patch)(W/patch), Kpad]: the Qwen2-VL processor's rescale,
    normalize and patchify (merge-window row order) in one launch."""
    H, W, C = img.shape
    assert C == 3 and img.dtype == torch.uint8 and img.is_contiguous() and lut.dtype == torch.float32 and lut.shape == (3, 256) and lut.is_contiguous()
    S = (H // patch) * (W // patch)
    if out is None:
        out = torch.empty(S, Kpad, dtype=torch.bfloat16, device=img.device)
    assert out.shape == (S, Kpad) and out.is_contiguous() and out.dtype == torch.bfloat16
    check(lib().td_qwen2_patchify_u8(ptr(img), H, W, ptr(lut), int(patch), int(merge), int(temporal), ptr(out), int(Kpad), stream_ptr()))
    return out


_resize_tables = {}                      # (in_size, out_size, filter) -> (numpy int32 [2 out + out ksize] = bounds | kk, ksize, the same memory as a torch tensor)
_resize_tables_lock = threading.Lock()   # the request builder's helper thread and the main thread both resize


def _resize_table(in_size, out_size, resample):
    import numpy as np
    key = (int(in_size), int(out_size), int(resample))
    with _resize_tables_lock:
        hit = _resize_tables.get(key)
    if hit is not None:
        return hit
    L = lib()
    ks = ctypes.c_int(0)
    check(L.td_resize_coeffs(key[0], key[1], key[2], None, None, ctypes.byref(ks)))
    tab = np.empty(2 * key[1] + key[1] * ks.value, dtype=np.int32)
    base = tab.ctypes.data
    check(L.td_resize_coeffs(key[0], key[1], key[2], ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * key[1]), ctypes.byref(ks)))
    host = torch.from_numpy(tab)
    tab.setflags(write=False)
    hit = (tab, ks.value, host)
    with _resize_tables_lock:
        if len(_resize_tables) >= 512:       # a dataset of arbitrary sizes must not grow the cache without bound
            _resize_tables.clear()
        hit = _resize_tables.setdefault(key, hit)
    return hit


def resize_coeffs(in_size, out_size, resample):
    """One axis' Pillow coefficient table (td_resize_coeffs, host only): (numpy int32 [2 * out_size + out_size * ksize] = bounds | kk, ksize),
    cached by (in_size, out_size, resample) under a lock; the array is shared between callers and read-only."""
    return _resize_table(in_size, out_size, resample)[:2]


def image_resize_u8(img, out_h, out_w, resample, out_channels=None, out=None):
    """PIL's Image.resize on the device: img uint8 [H, W, C] (or [H, W] = one channel), cuda, contiguous -> uint8 [out_h, out_w, out_channels or C],
    Pillow's bytes for resample 1 (LANCZOS), 2 (BILINEAR), 3 (BICUBIC).  C -> out_channels: 3 -> 3, 1 -> 1, 1 -> 3 ("L" replicated), 4 -> 3 ("RGBA"
    with alpha dropped), as convert("RGB") before the resize.  The host tables are cached; their device copy is made per call on the current stream
    ahead of the launch, so nothing on the device is shared between streams."""
    if img.dim() == 2:
        img = img[:, :, None]
    assert img.dim() == 3 and img.dtype == torch.uint8 and img.is_contiguous(), (img.shape, img.dtype)
    in_h, in_w, in_c = img.shape
    out_h, out_w = int(out_h), int(out_w)
    out_c = in_c if out_channels is None else int(out_channels)
    if out is None:
        out = torch.empty(max(out_h, 0), max(out_w, 0), out_c, dtype=torch.uint8, device=img.device)
    assert out.shape == (out_h, out_w, out_c) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == img.device
    horiz, vert = out_w != in_w, out_h != in_h
    parts, kh, kv = [], 0, 0
    if horiz:
        _, kh, th = _resize_table(in_w, out_w, resample)
        parts.append(th)
    if vert:
        _, kv, tv = _resize_table(in_h, out_h, resample)
        parts.append(tv)
    hb = hk = vb = vk = None
    if parts:
        dev_tab = (parts[0] if len(parts) == 1 else torch.cat(parts)).to(img.device)      # one upload for both axes
        base, o = dev_tab.data_ptr(), 0
        if horiz:
            hb, hk, o = ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * out_w), 4 * th.numel()
        if vert:
            vb, vk = ctypes.c_void_p(base + o), ctypes.c_void_p(base + o + 8 * out_h)
    tmp = torch.empty(in_h * out_w * out_c, dtype=torch.uint8, device=img.device) if horiz and vert else None
    check(lib().td_image_resize_u8(ptr(img), in_h, in_w, in_c, ptr(out), out_h, out_w, out_c, hb, hk, kh, vb, vk, kv, ptr(tmp), stream_ptr()))
    return out


def image_lut_chw_f32(img, lut, out=None):
    """img uint8 [H, W, C] (cuda, contiguous), lut fp32 [C, 256] (cuda) -> fp32 [C, H, W] = lut[c][img[y, x, c]]: a processor's rescale + normalize as
    its own table of the 256 pixel values per channel (td_image_lut_chw_f32)."""
    H, W, C = img.shape
    assert img.dtype == torch.uint8 and img.is_contiguous() and lut.dtype == torch.float32 and lut.shape == (C, 256) and lut.is_contiguous()
    if out is None:
        out = torch.empty(C, H, W, dtype=torch.float32, device=img.device)
    assert out.shape == (C, H, W) and out.dtype == torch.float32 and out.is_contiguous()
    check(lib().td_image_lut_chw_f32(ptr(img), H, W, C, ptr(lut), ptr(out), stream_ptr()))
    return out


def patchify(pix, p, Kpad):
    """pix [C,H,W] fp32|bf16 -> [(H/p)(W/p), Kpad] bf16."""
    C, H, W = pix.shape
    assert pix.is_contiguous() and pix.dtype in (torch.float32, torch.bfloat16)
    out = torch.empty((H // p) * (W // p), Kpad, dtype=torch.bfloat16, device=pix.device)
    check(lib().td_patchify_bf16(ptr(pix), int(pix.dtype == torch.float32), C, H, W, p, ptr(out), Kpad, stream_ptr()))
    return out


def cast_pad_rows(src, Kpad):
    rows, K = src.shape
    assert src.is_contiguous() and src.dtype in (torch.float32, torch.bfloat16)
    out = torch.empty(rows, Kpad, dtype=torch.bfloat16, device=src.device)
    check(lib().td_cast_pad_rows_bf16(ptr(src), int(src.dtype == torch.float32), rows, K, ptr(out), Kpad, stream_ptr()))
    return out


def vision_rope_table(pos, hd, theta=10000.0):
    """pos int32 [S,2] on the device -> (cos, sin) fp32 [S, hd/2]."""
    S = pos.shape[0]
    assert pos.dtype == torch.int32 and pos.is_contiguous() and pos.shape[1] == 2
    cos = torch.empty(S, hd // 2, dtype=torch.float32, device=pos.device)
    sin = torch.empty_like(cos)
    check(lib().td_vision_rope_table(ptr(pos), S, hd, float(theta), ptr(cos), ptr(sin), stream_ptr()))
    return cos, sin


# ---- fp8 operand path --------------------------------------------------------------------------------------------
def quant_rows_fp8(x):
    """bf16 [R,K] -> (uint8 e4m3 [R,K], fp32 scale [R])."""
    R, K = x.shape
    q = torch.empty(R, K, dtype=torch.uint8, device=x.device)
    s = torch.empty(R, dtype=torch.float32, device=x.device)
    check(lib().td_quant_rows_fp8(ptr(x), _rows(x), ptr(q), K, ptr(s), R, K, stream_ptr()))
    return q, s


def linear_fp8(xq, xs, wq, ws, bias=None, act=ACT_NONE, gate=None, res=None, out=None, tile_cfg=-1):
    M, K = xq.shape
    N = wq.shape[0]
    assert xq.dtype == torch.uint8 and wq.dtype == torch.uint8 and wq.shape[1] == K and wq.is_contiguous()
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=xq.device)
    check(lib().td_linear_fp8(ptr(xq), xq.stride(0), ptr(xs), ptr(wq), ptr(ws), ptr(bias), ptr(out), _rows(out), M, N, K, act,
                              ptr(gate), ptr(res), _rows(res) if res is not None else 0, tile_cfg, stream_ptr()))
    return out


def quant_rows_int8(x):
    """bf16 [R,K] -> (int8 [R,K], fp32 scale [R]): q = rint(x / s), s = max|x| / 127 per row."""
    R, K = x.shape
    q = torch.empty(R, K, dtype=torch.int8, device=x.device)
    s = torch.empty(R, dtype=torch.float32, device=x.device)
    check(lib().td_quant_rows_int8(ptr(x), _rows(x), ptr(q), K, ptr(s), R, K, stream_ptr()))
    return q, s


def linear_int8(xq, xs, wq, ws, bias=None, act=ACT_NONE, gate=None, res=None, out=None, tile_cfg=-1):
    M, K = xq.shape
    N = wq.shape[0]
    assert xq.dtype == torch.int8 and wq.dtype == torch.int8 and wq.shape[1] == K and wq.is_contiguous()
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=xq.device)
    check(lib().td_linear_int8(ptr(xq), xq.stride(0), ptr(xs), ptr(wq), ptr(ws), ptr(bias), ptr(out), _rows(out), M, N, K, act,
                               ptr(gate), ptr(res), _rows(res) if res is not None else 0, tile_cfg, stream_ptr()))
    return out


def norm_rows_quant_fp8(x, rms=False, eps=1e-6, w=None, split=0, shiftA=None, scaleA=None, shiftB=None, scaleB=None):
    R, D = x.shape
    q = torch.empty(R, D, dtype=torch.uint8, device=x.device)
    s = torch.empty(R, dtype=torch.float32, device=x.device)
    check(lib().td_norm_rows_quant_fp8(ptr(x), _rows(x), ptr(q), D, ptr(s), R, D, int(rms), float(eps), ptr(w), split,
                                       ptr(shiftA), ptr(scaleA), ptr(shiftB), ptr(scaleB), stream_ptr()))
    return q, s


# ---- int8 policy building blocks (include/thinkdiff_hip.h, same heading): thin wrappers; maxima travel as int32 tensors holding float bits ------
def _bytes2d(t):
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype in (torch.int8, torch.uint8), (t.shape, t.stride(), t.dtype)
    return t.stride(0)


def norm_rows_quant8(x, int8=True, q=None, rms=False, eps=1e-6, w=None, split=0, shiftA=None, scaleA=None, shiftB=None, scaleB=None,
                     smoothA=None, smoothB=None, extA=None, extB=None):
    """td_norm_rows_quant8: (q [rows, >= D + ext_n] int8 / e4m3 bytes, fp32 scale [rows]); q may be a caller's wider (pre-filled) buffer."""
    R, D = x.shape
    ext_n = 0 if extA is None else extA.numel()
    if q is None:
        q = torch.empty(R, D + ext_n, dtype=torch.int8 if int8 else torch.uint8, device=x.device)
    s = torch.empty(R, dtype=torch.float32, device=x.device)
    check(lib().td_norm_rows_quant8(ptr(x), _rows(x), ptr(q), _bytes2d(q), ptr(s), R, D, int(rms), float(eps), ptr(w), split,
                                    ptr(shiftA), ptr(scaleA), ptr(shiftB), ptr(scaleB), int(int8), ptr(smoothA), ptr(smoothB), ptr(extA), ptr(extB), ext_n, stream_ptr()))
    return q, s


def quant_rows8(x, int8=True, col_mul=None, want_amax=False, q=None):
    """td_quant_rows8: (q, fp32 scale [R], int32 float-bits row maxima [R] or None)."""
    R, K = x.shape
    if q is None:
        q = torch.empty(R, K, dtype=torch.int8 if int8 else torch.uint8, device=x.device)
    s = torch.empty(R, dtype=torch.float32, device=x.device)
    amax = torch.empty(R, dtype=torch.int32, device=x.device) if want_amax else None
    check(lib().td_quant_rows8(ptr(x), _rows(x), ptr(q), _bytes2d(q), ptr(s), R, K, int(int8), ptr(col_mul), ptr(amax), stream_ptr()))
    return q, s, amax


def col_amax(x, amax, rows=None):
    """td_col_amax_bf16 in place on amax (int32 float bits [K]) over the first `rows` rows of x."""
    R, K = x.shape
    assert amax.dtype == torch.int32 and amax.numel() == K and amax.is_contiguous()
    check(lib().td_col_amax_bf16(ptr(x), _rows(x), R if rows is None else rows, K, ptr(amax), stream_ptr()))
    return amax


def smooth_factors(amax_x, amax_w):
    """td_smooth_factors: (s fp32, 1 / s fp32, 1 / s bf16) from two int32 float-bits arrays."""
    n = amax_x.numel()
    assert amax_x.dtype == amax_w.dtype == torch.int32 and amax_w.numel() == n
    s = torch.empty(n, dtype=torch.float32, device=amax_x.device)
    inv = torch.empty_like(s)
    inv16 = torch.empty(n, dtype=torch.bfloat16, device=amax_x.device)
    check(lib().td_smooth_factors(ptr(amax_x), ptr(amax_w), n, ptr(s), ptr(inv), ptr(inv16), stream_ptr()))
    return s, inv, inv16


def q8_scales_from_amax(amax, margin):
    """td_q8_scales_from_amax: (scale, inv) fp32; amax (int32 float bits) is cleared in place."""
    n = amax.numel()
    assert amax.dtype == torch.int32 and amax.is_contiguous()
    scale = torch.empty(n, dtype=torch.float32, device=amax.device)
    inv = torch.empty_like(scale)
    check(lib().td_q8_scales_from_amax(ptr(amax), ptr(scale), ptr(inv), n, float(margin), stream_ptr()))
    return scale, inv


def ext_cols_int8(q, K, ext):
    """td_ext_cols_int8 in place on q int8 [rows, >= K + ext_n]; ext int32 [ext_n] on the device."""
    assert ext.dtype == torch.int32 and ext.is_contiguous()
    check(lib().td_ext_cols_int8(ptr(q), _bytes2d(q), q.shape[0], K, ptr(ext), ext.numel(), stream_ptr()))
    return q


class TdLinearQ8Problem(ctypes.Structure):
    """Mirror of `struct TdLinearQ8Problem` (include/thinkdiff_hip.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("xq", "x_scale", "wq", "w_scale", "bias", "q8", "q8_inv", "q8_amax", "q8_smooth")] + [("M", ctypes.c_int)]


def q8_problem(xq, xs, wq, ws, bias, q8, q8_inv, q8_amax, q8_smooth=None):
    """One problem of an int8-output Linear: xq int8 [M, K], wq int8 [N, K], q8 int8 [M, >= int8 columns], q8_amax int32 float bits [M]."""
    assert xq.dtype == torch.int8 and wq.dtype == torch.int8 and wq.is_contiguous() and wq.shape[1] == xq.shape[1] and q8_amax.dtype == torch.int32
    dp = lambda t: None if t is None else t.data_ptr()
    pr = TdLinearQ8Problem(dp(xq), dp(xs), dp(wq), dp(ws), dp(bias), dp(q8), dp(q8_inv), dp(q8_amax), dp(q8_smooth), xq.shape[0])
    pr._keep = (xq, xs, wq, ws, bias, q8, q8_inv, q8_amax, q8_smooth)
    return pr


def linear_int8_q8(pr, N, K, ldx, ldq8, act=ACT_NONE, tile_cfg=0):
    check(lib().td_linear_int8_q8(ctypes.byref(pr), ldx, ldq8, N, K, act, tile_cfg, stream_ptr()))


def linear_split_int8_q8(pr, N, K, ldx, ldq8, y0, act0, act1, n_split, tile_cfg=0):
    check(lib().td_linear_split_int8_q8(ctypes.byref(pr), ldx, ldq8, ptr(y0), _rows(y0), act0, act1, N, K, n_split, tile_cfg, stream_ptr()))
    return y0


def linear_grouped2_int8_q8(pr0, pr1, N, K, ldx, ldq8, act=ACT_NONE, tile_cfg=0):
    check(lib().td_linear_grouped2_int8_q8(ctypes.byref(pr0), ctypes.byref(pr1), ldx, ldq8, N, K, act, tile_cfg, stream_ptr()))


def attention_q8(q, k, v, q8, q8_inv, q8_amax, H, scale=None, q_prescaled=False, score_bound=0.0):
    """td_attention_q8: q, k, v bf16 [S, >= H*128] views, q8 int8 [Sq, >= H*128] (written in place), q8_amax int32 float bits [Sq] (max-accumulated)."""
    for t in (q, k, v):
        assert t.dim() == 2 and t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert k.stride() == v.stride() and q8_amax.dtype == torch.int32 and q8_inv.dtype == torch.float32
    if scale is None:
        scale = 128 ** -0.5
    check(lib().td_attention_q8(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(q8), _bytes2d(q8), ptr(q8_inv), ptr(q8_amax), q.shape[0], k.shape[0], H,
                                float(scale), 0, None, int(q_prescaled), float(score_bound), stream_ptr()))
    return q8


def attention_fp8_q8(q, k, v, q8, q8_inv, q8_amax, H, scale=None):
    """td_attention_fp8_q8: as attention_q8 over the e4m3 joint attention."""
    for t in (q, k, v):
        assert t.dim() == 2 and t.dtype == torch.bfloat16 and t.stride(1) == 1
    assert k.stride() == v.stride() and q8_amax.dtype == torch.int32 and q8_inv.dtype == torch.float32
    if scale is None:
        scale = 128 ** -0.5
    L = lib()
    ws = torch.empty(int(L.td_attention_fp8_workspace_bytes(q.shape[0], k.shape[0], H)), dtype=torch.uint8, device=q.device)
    check(L.td_attention_fp8_q8(ptr(q), q.stride(0), ptr(k), ptr(v), k.stride(0), ptr(q8), _bytes2d(q8), ptr(q8_inv), ptr(q8_amax), q.shape[0], k.shape[0], H,
                                float(scale), ptr(ws), stream_ptr()))
    return q8


def sample_top_p(logits, temperature, top_p, seed, offset, out=None):
    """logits bf16 [rows, vocab] (or [vocab]) -> int32 [rows] token ids on the device; no host synchronisation."""
    x = logits if logits.dim() == 2 else logits[None]
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    if out is None:
        out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    check(lib().td_sample_top_p_bf16(ptr(x), x.stride(0), x.shape[0], x.shape[1], float(temperature), float(top_p),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, ptr(out), stream_ptr()))
    return out


class TdSampleRow(ctypes.Structure):
    """One row's settings for td_sample_rows_bf16 (include/thinkdiff_hip.h; sizeof checked against td_sample_row_size() in tests)."""
    _fields_ = [("temperature", ctypes.c_float), ("top_p", ctypes.c_float), ("min_p", ctypes.c_float), ("repetition_penalty", ctypes.c_float),
                ("presence_penalty", ctypes.c_float), ("frequency_penalty", ctypes.c_float), ("top_k", ctypes.c_int), ("slot", ctypes.c_int),
                ("stream", ctypes.c_int), ("seed", ctypes.c_uint64)]


SAMPLE_ROW_DEFAULTS = dict(temperature=1.0, top_p=1.0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, top_k=-1,
                           slot=-1, stream=0, seed=0)


def pack_sample_rows(rows):
    """A list of dicts (keys of SAMPLE_ROW_DEFAULTS; missing keys take the default) -> CPU uint8 tensor [len(rows), sizeof(TdSampleRow)], the packed
    params operand of sample_rows / torch.ops.thinkdiff_hip.sample_rows."""
    arr = (TdSampleRow * len(rows))()
    for a, r in zip(arr, rows):
        unknown = set(r) - set(SAMPLE_ROW_DEFAULTS)
        if unknown:
            raise ThinkDiffHipError(f"pack_sample_rows: unknown field(s) {sorted(unknown)}")
        for k, d in SAMPLE_ROW_DEFAULTS.items():
            v = r.get(k, d)
            setattr(a, k, (int(v) & 0xFFFFFFFFFFFFFFFF) if k == "seed" else (float(v) if isinstance(d, float) else int(v)))
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).view(len(rows), ctypes.sizeof(TdSampleRow))


class Sampler:
    """td_sampler: the token history of n_slots sequences (prompt bitmap + uint16 generated-token counts per vocabulary entry, n_slots x vocab x
    2.25 bytes on the device) that the penalties of sample_rows read."""

    def __init__(self, n_slots, vocab, device=None):
        self.n_slots, self.vocab = int(n_slots), int(vocab)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        h = ctypes.c_void_p()
        self._destroy = lib().td_sampler_destroy      # (held here: __del__ may run while the interpreter tears the module down)
        with torch.cuda.device(self.device):
            check(lib().td_sampler_create(self.n_slots, self.vocab, ctypes.byref(h)))
        self._h = h

    @property
    def handle(self):
        return int(self._h.value or 0)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._destroy(h)

    __del__ = close

    def reset_slot(self, slot, prompt_ids=None):
        """Clear the slot's history and mark `prompt_ids` (a sequence or an int32 device tensor; ids outside the vocabulary are ignored)."""
        ids = None
        if prompt_ids is not None and len(prompt_ids):
            ids = prompt_ids if torch.is_tensor(prompt_ids) else torch.tensor(list(prompt_ids), dtype=torch.int32)
            ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        check(lib().td_sampler_reset_slot(self._h, int(slot), ptr(ids), 0 if ids is None else ids.numel(), stream_ptr()))

    def read_counts(self, slot):
        out = torch.empty(self.vocab, dtype=torch.int32, device=self.device)
        check(lib().td_sampler_read_counts(self._h, int(slot), ptr(out), stream_ptr()))
        return out

    def read_prompt_mask(self, slot):
        out = torch.empty(self.vocab, dtype=torch.uint8, device=self.device)
        check(lib().td_sampler_read_prompt_mask(self._h, int(slot), ptr(out), stream_ptr()))
        return out

    def set_counts(self, slot, counts):
        c = counts.to(device=self.device, dtype=torch.int32).contiguous()
        assert c.numel() == self.vocab
        check(lib().td_sampler_set_counts(self._h, int(slot), ptr(c), stream_ptr()))


def sampler_create(n_slots, vocab, device=None):
    return Sampler(n_slots, vocab, device)


def sample_rows(logits, params, offsets, sampler=None, update_state=False, out=None):
    """td_sample_rows_bf16: logits bf16 [rows, vocab] -> int32 [rows] ids, each row under its own settings.  params: the packed uint8
    [rows, sizeof(TdSampleRow)] tensor (pack_sample_rows) or a list of dicts; offsets: int64 [rows] tensor, a list, or one int for every row.
    Host-side operands are uploaded here; device tensors are used as they are (no host synchronisation)."""
    x = logits if logits.dim() == 2 else logits[None]
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    rows = x.shape[0]
    if not torch.is_tensor(params):
        params = pack_sample_rows(params)
    params = params.to(x.device).contiguous()
    if params.dtype != torch.uint8 or params.numel() != rows * ctypes.sizeof(TdSampleRow):
        raise ThinkDiffHipError(f"sample_rows: params must hold {rows} packed TdSampleRow structs ({rows * ctypes.sizeof(TdSampleRow)} bytes), got {params.numel()}")
    if not torch.is_tensor(offsets):
        offsets = torch.tensor([int(offsets)] * rows if isinstance(offsets, int) else [int(o) for o in offsets], dtype=torch.int64)
    offsets = offsets.to(device=x.device, dtype=torch.int64).contiguous()
    if offsets.numel() != rows:
        raise ThinkDiffHipError(f"sample_rows: {offsets.numel()} offsets for {rows} rows")
    if out is None:
        out = torch.empty(rows, dtype=torch.int32, device=x.device)
    h = None if sampler is None else (sampler._h if isinstance(sampler, Sampler) else ctypes.c_void_p(int(sampler)))
    check(lib().td_sample_rows_bf16(h, ptr(x), x.stride(0), rows, x.shape[1], ptr(params), ptr(offsets), int(bool(update_state)), ptr(out), stream_ptr()))
    return out


MAX_LOGIT_BIAS = 1024      # TD_MAX_LOGIT_BIAS
MAX_LOGPROBS = 20          # TD_MAX_LOGPROBS


class LogitEdits:
    """td_logit_edits: n_slots edit slots over one vocabulary (per slot a ban bitmap, a bias bitmap and a sorted table of at most 1024
    (token, fp32 bias) pairs; n_slots x (2 x vocab / 8 + 8196) bytes on the device, 11.8 MB at 256 x 152 064) that sample_rows_edit applies to the
    logits in front of the penalties.  Every setter is stream-ordered and does not synchronise."""

    def __init__(self, n_slots, vocab, device=None):
        self.n_slots, self.vocab = int(n_slots), int(vocab)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        h = ctypes.c_void_p()
        self._destroy = lib().td_logit_edits_destroy      # (held here: __del__ may run while the interpreter tears the module down)
        with torch.cuda.device(self.device):
            check(lib().td_logit_edits_create(self.n_slots, self.vocab, ctypes.byref(h)))
        self._h = h

    @property
    def handle(self):
        return int(self._h.value or 0)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._destroy(h)

    __del__ = close

    def _ids(self, ids):
        t = ids if torch.is_tensor(ids) else torch.tensor([int(i) for i in ids], dtype=torch.int32)
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def reset_slot(self, slot):
        """Clear the slot's bans and biases."""
        check(lib().td_logit_edits_reset_slot(self._h, int(slot), stream_ptr()))

    def set_bias(self, slot, bias):
        """Replace the slot's bias table: `bias` is a dict token -> value or a sequence of (token, value) pairs, at most 1024, host side (the library
        sorts them; a duplicate id or an id outside the vocabulary is refused; NaN counts as 0, +-inf is honoured)."""
        items = list(bias.items()) if hasattr(bias, "items") else [tuple(p) for p in bias]
        n = len(items)
        ids = (ctypes.c_int32 * max(n, 1))(*[int(t) for t, _ in items])
        vals = (ctypes.c_float * max(n, 1))(*[float(v) for _, v in items])
        check(lib().td_logit_edits_set_bias(self._h, int(slot), ctypes.cast(ids, ctypes.c_void_p), ctypes.cast(vals, ctypes.c_void_p), n, stream_ptr()))

    def ban(self, slot, ids, on=True):
        """Set (or, on=False, clear) the ban on `ids` (a sequence or an int32 device tensor; ids outside the vocabulary are ignored)."""
        t = self._ids(ids)
        check(lib().td_logit_edits_ban(self._h, int(slot), ptr(t) if t.numel() else None, t.numel(), int(bool(on)), stream_ptr()))

    def allow_only(self, slot, ids):
        """Ban every token except `ids` (replaces the slot's bans, keeps its biases)."""
        t = self._ids(ids)
        check(lib().td_logit_edits_allow_only(self._h, int(slot), ptr(t) if t.numel() else None, t.numel(), stream_ptr()))

    def read(self, slot):
        """-> (banned uint8 [vocab], bias fp32 [vocab]) on the device (tests and debugging)."""
        banned = torch.empty(self.vocab, dtype=torch.uint8, device=self.device)
        bias = torch.empty(self.vocab, dtype=torch.float32, device=self.device)
        check(lib().td_logit_edits_read(self._h, int(slot), ptr(banned), ptr(bias), stream_ptr()))
        return banned, bias


def logit_edits_create(n_slots, vocab, device=None):
    return LogitEdits(n_slots, vocab, device)


def sample_rows_edit(logits, params, offsets, sampler=None, update_state=False, edits=None, edit_slots=None, out=None):
    """td_sample_rows_edit_bf16: sample_rows with the edits of slot edit_slots[row] (an int32 [rows] tensor, a list, or one int for every row; -1 = no
    edits) applied to each row's logits in front of the penalties.  edits None: sample_rows."""
    if edits is None:
        return sample_rows(logits, params, offsets, sampler, update_state, out)
    x = logits if logits.dim() == 2 else logits[None]
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    rows = x.shape[0]
    if not torch.is_tensor(params):
        params = pack_sample_rows(params)
    params = params.to(x.device).contiguous()
    if params.dtype != torch.uint8 or params.numel() != rows * ctypes.sizeof(TdSampleRow):
        raise ThinkDiffHipError(f"sample_rows_edit: params must hold {rows} packed TdSampleRow structs ({rows * ctypes.sizeof(TdSampleRow)} bytes), got {params.numel()}")
    if not torch.is_tensor(offsets):
        offsets = torch.tensor([int(offsets)] * rows if isinstance(offsets, int) else [int(o) for o in offsets], dtype=torch.int64)
    offsets = offsets.to(device=x.device, dtype=torch.int64).contiguous()
    if edit_slots is None:
        edit_slots = -1
    if not torch.is_tensor(edit_slots):
        edit_slots = torch.tensor([int(edit_slots)] * rows if isinstance(edit_slots, int) else [int(s) for s in edit_slots], dtype=torch.int32)
    edit_slots = edit_slots.to(device=x.device, dtype=torch.int32).contiguous()
    if offsets.numel() != rows or edit_slots.numel() != rows:
        raise ThinkDiffHipError(f"sample_rows_edit: {offsets.numel()} offsets and {edit_slots.numel()} edit slots for {rows} rows")
    if out is None:
        out = torch.empty(rows, dtype=torch.int32, device=x.device)
    h = None if sampler is None else (sampler._h if isinstance(sampler, Sampler) else ctypes.c_void_p(int(sampler)))
    eh = edits._h if isinstance(edits, LogitEdits) else ctypes.c_void_p(int(edits))
    check(lib().td_sample_rows_edit_bf16(h, eh, ptr(edit_slots), ptr(x), x.stride(0), rows, x.shape[1], ptr(params), ptr(offsets), int(bool(update_state)),
                                         ptr(out), stream_ptr()))
    return out


def logprobs_rows(logits, ids, n_top, top_cap=MAX_LOGPROBS, out=None):
    """td_logprobs_rows_bf16 on RAW logits bf16 [rows, vocab]: ids int32 [rows] (the chosen tokens), n_top int32 [rows] (a tensor, a list or one int;
    -1 skips a row) -> (lp_sampled fp32 [rows], rank int32 [rows], top_ids int32 [rows, top_cap], top_lp fp32 [rows, top_cap]).  `out`: that tuple of
    tensors to write into (skipped rows leave theirs untouched); otherwise fresh ones, pre-filled with lp -inf, rank 0 and id -1."""
    x = logits if logits.dim() == 2 else logits[None]
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    rows, top_cap = x.shape[0], int(top_cap)
    ids = (ids if torch.is_tensor(ids) else torch.tensor([int(i) for i in ids], dtype=torch.int32)).to(device=x.device, dtype=torch.int32).contiguous()
    if not torch.is_tensor(n_top):
        n_top = torch.tensor([int(n_top)] * rows if isinstance(n_top, int) else [int(v) for v in n_top], dtype=torch.int32)
    n_top = n_top.to(device=x.device, dtype=torch.int32).contiguous()
    if ids.numel() != rows or n_top.numel() != rows:
        raise ThinkDiffHipError(f"logprobs_rows: {ids.numel()} ids and {n_top.numel()} n_top for {rows} rows")
    if out is None:
        out = (torch.full((rows,), float("-inf"), dtype=torch.float32, device=x.device), torch.zeros(rows, dtype=torch.int32, device=x.device),
               torch.full((rows, max(top_cap, 0)), -1, dtype=torch.int32, device=x.device),
               torch.full((rows, max(top_cap, 0)), float("-inf"), dtype=torch.float32, device=x.device))
    lp, rank, top_ids, top_lp = out
    check(lib().td_logprobs_rows_bf16(ptr(x), x.stride(0), rows, x.shape[1], ptr(ids), ptr(n_top), top_cap, ptr(lp), ptr(rank),
                                      ptr(top_ids) if top_cap > 0 else None, ptr(top_lp) if top_cap > 0 else None, stream_ptr()))
    return lp, rank, top_ids, top_lp


def redux_compose(text, image, scales, T=None, D=None, device=None, out=None):
    """FLUX.1 Redux (td_redux_compose_bf16): out[T + S, D] = sum over b of bf16(bf16(scales[b]) * [text[b] | image[b]]), fp32 sum in index order,
    one rounding.  text [1 or B, T, D] or None (T rows of +0.0, `T=` gives the count), image [B, S, D] or None (S = 0); both contiguous bf16.
    A text of batch 1 with B > 1 is shared by every stream and still added B times.  With neither, `D=` and `device=` size the zero rows.
    `out` may be a 2-D view whose row stride exceeds D."""
    scales = [float(s) for s in scales]
    B = len(scales)
    ref = image if image is not None else text
    if ref is not None:
        D, device = ref.shape[-1], ref.device
    elif D is None or device is None or not T:
        raise ThinkDiffHipError("redux_compose: without text and image, T=, D= and device= must size the zero rows")
    for name, t in (("text", text), ("image", image)):
        if t is not None and not (t.dim() == 3 and t.dtype == torch.bfloat16 and t.is_contiguous() and t.shape[2] == D and t.device == device):
            raise ThinkDiffHipError(f"redux_compose: {name} must be a contiguous bf16 [batch, rows, {D}] tensor on {device}, got {tuple(t.shape)} {t.dtype}")
    if image is not None and image.shape[0] != B:
        raise ThinkDiffHipError(f"redux_compose: image has batch {image.shape[0]}, {B} scales were given")
    if text is not None and text.shape[0] not in (1, B):
        raise ThinkDiffHipError(f"redux_compose: text has batch {text.shape[0]}, expected 1 or {B}")
    T = text.shape[1] if text is not None else int(T or 0)
    S = image.shape[1] if image is not None else 0
    if out is None:
        out = torch.empty((T + S, D), dtype=torch.bfloat16, device=device)
    assert out.shape[0] == T + S and out.shape[1] >= D and out.is_cuda
    tbs = text.stride(0) if text is not None and text.shape[0] > 1 else 0
    ibs = image.stride(0) if image is not None else 0
    check(lib().td_redux_compose_bf16(ptr(text), tbs, T, ptr(image), ibs, S, (ctypes.c_float * B)(*scales), B, D, ptr(out), _rows(out), stream_ptr()))
    return out


def kernel_source_digest() -> str:
    """sha256 over the kernel sources of this tree (csrc/*.hip, csrc/*.h, include/thinkdiff_hip.h; names and contents, sorted): parity records
    written on the GPU box carry it, and bench.py quotes a record only when it was measured on the sources it is running."""
    import glob
    import hashlib
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(pkg, "csrc", "*.hip")) + glob.glob(os.path.join(pkg, "csrc", "*.h")))
    files.append(os.path.join(os.path.dirname(pkg), "include", "thinkdiff_hip.h"))
    h = hashlib.sha256()
    for fn in files:
        h.update(os.path.basename(fn).encode() + b"\0")
        with open(fn, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()
