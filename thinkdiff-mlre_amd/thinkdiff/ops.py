"""`torch.ops.thinkdiff_hip.*`: the custom-op layer of the MI355X hot path (last row).

The ops are registered by a shared library -- `lib/libthinkdiff_torch_ops.so`, built by `make` from `csrc_torch/torch_ops.cpp`
(TORCH_LIBRARY + TORCH_LIBRARY_IMPL for the "CUDA" = HIP dispatch key) -- whose kernels hand raw device pointers to the C ABI of
`libthinkdiff_hip.so` (include/thinkdiff_hip.h).  Conventions: tensors are borrowed (caller owns, device-resident, innermost
stride 1), outputs are allocated by the PyTorch caching allocator on the current HIP stream, nothing synchronises, a rejected
argument is a `RuntimeError` carrying `td_last_error()`, one process per GPU.  There is NO CPU / Meta / composite kernel: calling
an op with host tensors fails in the dispatcher instead of quietly computing somewhere else, and importing this module without the
library raises.

    import thinkdiff.ops                      # loads the library (idempotent)
    y = torch.ops.thinkdiff_hip.linear(x, w, b, 0, None, None)

Op                         replaces in the reference's stack (details: include/thinkdiff_hip.h)
linear / aligner_mlp2x     nn.Linear (+bias/act/gate/residual), the ThinkDiff aligner mm_projector
attention                  F.scaled_dot_product_attention on token-major fused projections (joint or causal GQA)
norm_rows                  LayerNorm / RMSNorm rows (+ adaLN modulation)
qk_norm_rope_              per-head QK-RMSNorm + rotary embedding, in place
euler_step_                FlowMatchEulerDiscreteScheduler.step, in place
flux_pack_latents / flux_unpack_latents, cls_avgpool2, sample_top_p
sample_rows                per-request sampler: penalties, top-k, top-p, min-p per row (`state` = a thinkdiff._hip.Sampler handle or None)
sample_rows_edit           sample_rows with a per-row edit of the logits in front of the penalties: bans, allowed ids and logit_bias (`edits` = a
                           thinkdiff._hip.LogitEdits handle or None, `edit_slots` = int32 [rows], -1 = none)
logprobs_rows              the chosen token's logprob and rank and the top-n logprobs of each row of RAW logits (vLLM's `logprobs`), no sort
flux_forward_ / flux_denoise_ / flux_denoise_multi_   FluxTransformer2DModel.forward and the pipeline's denoising loop, on a prepared engine
                           (`engine` = the td_flux* handle thinkdiff.models.flux_transformer holds); tensors are checked against the
                           extents the prepared context expects (td_flux_prepared_shape)
vae_decode_u8              AutoencoderKL.decode + VaeImageProcessor.postprocess on a td_vae* engine
attention_fp8              the joint attention with QK^T / P.V on the e4m3 MFMA
vae_encode_moments         VaeImageProcessor.preprocess + AutoencoderKL.encode (posterior parameters) on a td_vae_enc* engine
vae_latents_from_moments   posterior sample / mode, the img2img pipeline's shift / scale, scale_noise and _pack_latents, fused
flux_inpaint_step_         FluxInpaintPipeline's step: scheduler.step + scale_noise of the image latents + mask blend, fused, in place
flux_inpaint_mask          the inpainting mask's binarize, F.interpolate(nearest) to the latent size, repeat and _pack_latents, fused
flux_denoise_inpaint_ / flux_denoise_multi_inpaint_   the inpainting denoise loop (flux_denoise_ / flux_denoise_multi_ with that step)
flux_set_reference_tokens  FluxKontextPipeline's per-step torch.cat of the reference-image latents / ids behind the latents, once per image
flux_cfg_step_             true classifier-free guidance (neg + scale * (pos - neg)) + scheduler.step, fused, in place
flux_denoise_cfg_          the denoise loop under true CFG: both conditionings per step on two prepared contexts, then flux_cfg_step_
flux_residual_inject_      FluxTransformer2DModel's `hidden_states + controlnet_block_samples[..]` with the ControlNet's `* conditioning_scale`, fused, in place
flux_residual_inject_multi_   the same under FluxMultiControlNetModel: the scaled samples of 1 .. 4 ControlNets summed in bf16 in list order, then added, one launch
block_cache_head / block_cache_tail   diffusers' First Block Cache arithmetic: the first block's residual with the two sums of its
                           `(r - r_prev).abs().mean() / r_prev.abs().mean()` test taken deterministically (no atomics), and the tail difference
lora_merge / lora_merge_   peft's `weight + scaling * (lora_B @ lora_A)` for up to 8 pairs at once, fp32 accumulation, one rounding
lora_rows_                 the UNMERGED form (vLLM's `enable_lora` with a LoRARequest per request): every row under an adapter of its own, that adapter's
                           `scale * lora_B(lora_A(x))` added behind a base Linear's output in place, 1 to 3 output segments per call, one rounding
flux_lora_load / flux_lora_set_adapters / flux_lora_delete / flux_read_param   diffusers' load_lora_weights / set_adapters / delete_adapters
                           (empty name: unload_lora_weights) on the engine's merged weights, and the effective parameter read back; the last
                           three take no tensor, so they alone are registered for every backend (they only reach the engine handle)
ip_attention / ip_attention_   FluxIPAdapterJointAttnProcessor2_0's image-prompt branch: the fused QK-RMSNorm of the un-rotated query, SDPA against
                           the adapter's few keys (true row maximum, masked padding) and `scale *`, written or accumulated
flux_ip_adapter_load_param / flux_set_ip_image_embeds / flux_ip_read   diffusers' load_ip_adapter weights and `ip_adapter_image_embeds` of one
                           image on an engine context (projection + every block's to_k_ip / to_v_ip, once), and the tokens / K / V read back
redux_compose              FluxPriorReduxPipeline's `cat([text, image_embeds], 1) * scale[:, None, None]` and `sum(dim=0)` over the images of one call, fused:
                           bf16 products, fp32 sum in index order, one rounding
image_resize_u8            PIL's `Image.resize` (LANCZOS / BILINEAR / BICUBIC, with `convert("RGB")` of "L" / "RGBA" folded in) on a uint8 HWC image: Pillow's
                           fixed-point horizontal and vertical passes as two kernels over host-made coefficient tables, the same bytes
quant_weight_rows_e4m3 / linear_w8   weight-only fp8 of an nn.Linear (vLLM's `quantization="fp8"` on the LVLM): e4m3 bytes with one power-of-two scale per
                           output row (bytes, scales and the dequantised bf16 weight, which is exact), and the Linear of up to 64 rows that streams the bytes
quant_weight_rows_mxfp4 / dequant_rows_mxfp4 / linear_w4   weight-only OCP MXFP4 of an nn.Linear (vLLM's `quantization="mxfp4"` on the LVLM): e2m1 nibbles (element 2j
                           in the low nibble of byte j) with one e8m0 scale byte per 32 weights of a row, back to bf16 (exact), and the Linear of up to 64 rows
                           that streams the nibbles
repack_int4 / dequant_rows_int4 / linear_i4   the grouped int4 of AWQ / GPTQ checkpoints (asymmetric uint4, one fp16 scale and one 4-bit zero point per group of
                           32 / 64 / 128 weights of a row): one checkpoint Linear (layout 0 = AutoAWQ "GEMM", 1 = AutoGPTQ, 3 = AutoGPTQ "gptq_v2") repacked into the
                           device layout, that layout back to bf16 (bf16_rne((q - z) s): one rounding), and the Linear of up to 64 rows that streams the nibbles
kv_quant_rows_e4m3 / kv_dequant_rows_e4m3 / attention_decode_kv8   the e4m3 KV cache of the LVLM's decode engine (vLLM's `kv_cache_dtype="fp8"`): e4m3 bytes with one
                           power-of-two scale per 128-wide head vector of a cache row, back to bf16 (exact), and the decode attention that reads bytes + scales
kv_fork_rows               the first n_rows rows of one slot of a cache plane copied to many slots in one launch, each source chunk loaded once (what vLLM's
                           `n` / `best_of` share through block tables is a copy here: the slots are a fixed partition); in place, any dtype
kv_gather_rows             row j of a launch takes the first n_rows[j] rows of the slot of row copy_src[j], a DEVICE int32 tensor (-1: nothing): the reordering of
                           cache slots behind a beam-search step, with no host round trip; in place, any dtype
beam_select                one beam-search step on the device (vLLM's `LLM.beam_search` loop): the next W beams out of W x 2W candidates (logprobs_rows with
                           n_top = 2W), EOS candidates set aside as finishers, and a slot-stable placement whose copies kv_gather_rows does in one launch
attention_verify / spec_accept   speculative decoding (vLLM's `speculative_config`, method "ngram"): the decode attention of a verify step -- up to 8 query rows per
                           sequence, bf16 or e4m3 cache; through this op one workgroup per row, bit-equal to the single-row kernel (the multi-row kernel is
                           routed by td_attention_verify_ex) -- and the accept rule: the sampled tokens up to the first wrong guess
attention_prefix_segments  context attention (vLLM's automatic prefix caching needs it): packed causal query segments, each over the key range of its own cache
                           slot -- the rows of its cached prefix and its own -- in one launch of the tile kernel
"""
import os

import torch

from . import _hip

OPS_LIB_PATH = os.path.join(os.path.dirname(_hip.LIB_PATH), "libthinkdiff_torch_ops.so")

# the schemas csrc_torch/torch_ops.cpp defines (tests compare them with what the dispatcher reports)
SCHEMAS = {
    "linear": "(Tensor x, Tensor w, Tensor? bias, int act, Tensor? gate, Tensor? res) -> Tensor",
    "aligner_mlp2x": "(Tensor x, Tensor w0, Tensor b0, Tensor w2, Tensor b2, Tensor norm_w, float eps, bool fp32_norm) -> Tensor",
    "attention": "(Tensor q, Tensor k, Tensor v, int Hq, int Hkv, float scale, bool causal) -> Tensor",
    "norm_rows": "(Tensor x, bool rms, float eps, Tensor? w, int split, Tensor? shiftA, Tensor? scaleA, Tensor? shiftB, Tensor? scaleB) -> Tensor",
    "qk_norm_rope_": "(Tensor(a!) qkv, int Hq, int Hk, int q_col, int k_col, Tensor cos, Tensor sin, int split, Tensor? wqA, Tensor? wkA, Tensor? wqB, Tensor? wkB, float eps, bool rotate_half) -> Tensor(a!)",
    "euler_step_": "(Tensor(a!) x, Tensor v, float dt) -> Tensor(a!)",
    "flux_pack_latents": "(Tensor latents) -> Tensor",
    "flux_unpack_latents": "(Tensor packed, int C, int H, int W, float div, float add) -> Tensor",
    "cls_avgpool2": "(Tensor tokens) -> Tensor",
    "sample_top_p": "(Tensor logits, float temperature, float top_p, int seed, int offset) -> Tensor",
    "sample_rows": "(Tensor logits, Tensor params, Tensor offsets, int? state, bool update_state) -> Tensor",
    "sample_rows_edit": "(Tensor logits, Tensor params, Tensor offsets, int? state, bool update_state, int? edits, Tensor? edit_slots) -> Tensor",
    "logprobs_rows": "(Tensor logits, Tensor ids, Tensor n_top, int top_cap) -> (Tensor, Tensor, Tensor, Tensor)",
    "flux_forward_": "(int engine, Tensor latents, int step, Tensor(a!) velocity) -> Tensor(a!)",
    "flux_denoise_": "(int engine, Tensor(a!) latents, float[] sigmas) -> Tensor(a!)",
    "flux_denoise_multi_": "(int[] engines, Tensor(a!)[] latents, float[] sigmas, int[] streams) -> ()",
    "vae_decode_u8": "(int engine, Tensor packed, int h, int w, float scaling_factor, float shift_factor) -> Tensor",
    "attention_fp8": "(Tensor q, Tensor k, Tensor v, int H, float scale) -> Tensor",
    "vae_encode_moments": "(int engine, Tensor image, int H, int W) -> Tensor",
    "vae_latents_from_moments": "(Tensor moments, Tensor? eps, Tensor? noise, float sigma, float scaling_factor, float shift_factor, int h, int w) -> Tensor",
    "flux_inpaint_step_": "(Tensor(a!) x, Tensor v, Tensor image_latents, Tensor? noise, Tensor mask, float dt, float sigma_next) -> Tensor(a!)",
    "flux_inpaint_mask": "(Tensor mask, int C) -> Tensor",
    "flux_denoise_inpaint_": "(int engine, Tensor(a!) latents, float[] sigmas, Tensor image_latents, Tensor noise, Tensor mask) -> Tensor(a!)",
    "flux_set_reference_tokens": "(int engine, Tensor ref_latents, Tensor ref_ids) -> ()",
    "flux_cfg_step_": "(Tensor(a!) x, Tensor v_pos, Tensor v_neg, float scale, float dt) -> Tensor(a!)",
    "flux_residual_inject_": "(Tensor(a!) h, Tensor r, float scale) -> Tensor(a!)",
    "flux_residual_inject_multi_": "(Tensor(a!) h, Tensor[] r, float[] scales) -> Tensor(a!)",
    "block_cache_head": "(Tensor h1, Tensor h0, Tensor? r_prev) -> (Tensor, Tensor)",
    "block_cache_tail": "(Tensor a, Tensor b) -> Tensor",
    "flux_denoise_cfg_": "(int engine_pos, int engine_neg, Tensor(a!) latents, float[] sigmas, float scale) -> Tensor(a!)",
    "flux_denoise_multi_inpaint_": "(int[] engines, Tensor(a!)[] latents, float[] sigmas, Tensor[] image_latents, Tensor[] noise, Tensor[] mask, int[] streams) -> ()",
    "lora_merge": "(Tensor w, Tensor[] A, Tensor[] B, float[] scales) -> Tensor",
    "lora_merge_": "(Tensor(a!) w, Tensor[] A, Tensor[] B, float[] scales) -> Tensor(a!)",
    "lora_rows_": "(Tensor x, Tensor row_adapter, Tensor[] A, Tensor[] B, int[] pair, float[] scales, Tensor(a!)[] ys) -> ()",
    "flux_read_param": "(int engine, str name) -> Tensor",
    "flux_lora_load": "(int engine, str adapter, str param, Tensor A, Tensor B, float scale) -> ()",
    "flux_lora_set_adapters": "(int engine, str[] names, float[] weights) -> ()",
    "flux_lora_delete": "(int engine, str adapter) -> ()",
    "ip_attention": "(Tensor q, Tensor k, Tensor v, int H, Tensor? norm_w, float eps, float out_scale) -> Tensor",
    "ip_attention_": "(Tensor(a!) o, Tensor q, Tensor k, Tensor v, int H, Tensor? norm_w, float eps, float out_scale, bool accumulate) -> Tensor(a!)",
    "flux_ip_adapter_load_param": "(int engine, int slot, str name, Tensor data) -> ()",
    "flux_set_ip_image_embeds": "(int engine, int slot, Tensor embeds) -> ()",
    "flux_ip_read": "(int engine, int slot, int block, int which) -> Tensor",
    "redux_compose": "(Tensor? text, Tensor? image, float[] scales, int text_rows) -> Tensor",
    "image_resize_u8": "(Tensor img, int out_h, int out_w, int resample, int? out_channels) -> Tensor",
    "quant_weight_rows_e4m3": "(Tensor w) -> (Tensor, Tensor, Tensor)",
    "linear_w8": "(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias, int act, Tensor? gate, Tensor? res) -> Tensor",
    "quant_weight_rows_mxfp4": "(Tensor w) -> (Tensor, Tensor, Tensor)",
    "dequant_rows_mxfp4": "(Tensor packed, Tensor scales) -> Tensor",
    "linear_w4": "(Tensor x, Tensor packed, Tensor scales, Tensor? bias, int act, Tensor? gate, Tensor? res) -> Tensor",
    "repack_int4": "(int layout, Tensor qweight, Tensor qzeros, Tensor scales, int group_size) -> (Tensor, Tensor, Tensor)",
    "dequant_rows_int4": "(Tensor packed, Tensor scales, Tensor zeros, int group_size) -> Tensor",
    "linear_i4": "(Tensor x, Tensor packed, Tensor scales, Tensor zeros, int group_size, Tensor? bias, int act, Tensor? gate, Tensor? res) -> Tensor",
    "kv_quant_rows_e4m3": "(Tensor kv, int heads) -> (Tensor, Tensor, Tensor)",
    "kv_dequant_rows_e4m3": "(Tensor q, Tensor scale) -> Tensor",
    "attention_decode_kv8": "(Tensor q, Tensor k8, Tensor v8, Tensor k_scale, Tensor v_scale, Tensor? kv_lens, int Hq, int Hkv, float scale) -> Tensor",
    "kv_fork_rows": "(Tensor(a!) plane, int slot_rows, int src_slot, int[] dst_slots, int n_rows) -> ()",
    "kv_gather_rows": "(Tensor(a!) plane, int slot_rows, int[] slots, Tensor copy_src, int[] n_rows) -> ()",
    "beam_select": "(Tensor top_ids, Tensor top_lp, Tensor cum_in, Tensor rank_in, int W, int n_in, int eos, Tensor(a!) token, Tensor(b!) cum_out, Tensor(c!) rank_out, "
                   "Tensor(d!) copy_src, Tensor(e!) parent, Tensor(f!) fin_flag, Tensor(g!) fin_cum) -> ()",
    "attention_verify": "(Tensor q, Tensor k, Tensor v, Tensor? k_scale, Tensor? v_scale, Tensor seq_row0, Tensor seq_rows, Tensor seq_len0, Tensor seq_slot, int Hq, int Hkv, "
                        "float scale) -> Tensor",
    "spec_accept": "(Tensor sampled, Tensor fed, Tensor seq_row0, Tensor seq_rows) -> (Tensor, Tensor)",
    "attention_prefix_segments": "(Tensor q, Tensor k, Tensor v, Tensor seg_starts, Tensor kv_row0, Tensor kv_lens, int max_q_len, int max_kv_len, int Hq, int Hkv, "
                                 "float scale) -> Tensor",
}

_loaded = False


def register():
    """Load libthinkdiff_torch_ops.so once per process (its static initialisers define the `thinkdiff_hip` namespace)."""
    global _loaded
    if not _loaded:
        if not os.path.exists(OPS_LIB_PATH):
            raise _hip.ThinkDiffHipError(f"{OPS_LIB_PATH} not found: build it with `make -C thinkdiff-mlre_amd` "
                                         "(or __graft_entry__.build()); there is no Python-side stand-in for the op layer")
        torch.ops.load_library(OPS_LIB_PATH)
        _loaded = True
    return torch.ops.thinkdiff_hip


register()
