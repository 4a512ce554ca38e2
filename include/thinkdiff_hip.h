/* thinkdiff_hip.h — C ABI of the MI355X-native ThinkDiff hot path (libthinkdiff_hip.so).
 *
 * The reference (avi22bhattacharya/ThinkDiff-mlre) has no native boundary: its hot path runs inside
 * diffusers / transformers / vLLM Python calls.  Each entry point below names the reference call it
 * replaces (path:line relative to the reference tree, or [ext] for the pinned third-party package
 * the reference calls into).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - every `const void*` / `void*` tensor argument is a DEVICE pointer (HBM), 16-byte aligned,
 *    borrowed for the duration of the call; bf16 tensors are raw uint16 bit patterns, row-major;
 *  - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work and never synchronise (exceptions, by
 *    purpose: td_*_create / td_flux_set_precision allocate, td_flux_trace_end reads its events back);
 *  - return value: TD_OK or an error code; td_last_error() returns a thread-local message;
 *  - no entry point allocates device memory except td_flux_create / td_*_create (workspaces are
 *    sized once at creation), so every call is hipGraph-capturable.
 */
#ifndef THINKDIFF_HIP_H
#define THINKDIFF_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { TD_OK = 0, TD_ERR_INVALID = 2, TD_ERR_HIP = 3 };
/* activation codes for td_linear_bf16 */
enum { TD_ACT_ID_NONE = 0, TD_ACT_ID_GELU_TANH = 1, TD_ACT_ID_GELU_ERF = 2, TD_ACT_ID_SILU = 3, TD_ACT_ID_QUICK_GELU = 4 };

const char* td_last_error(void);
int td_abi_version(void);

/* y[M,N] = act(x[M,K] . w[N,K]^T + bias) (* gate[N]) (+ res[M,N])      bf16 in/out, fp32 accumulate.
 * Replaces torch.nn.Linear (+ fused neighbours) wherever the reference's third-party stacks call it:
 * aligner mm_projector[0..2] (thinkdiff/models/blip_vision_t5_decoder.py:44-47), FLUX
 * to_q/k/v, to_out, ff, proj_mlp, proj_out [ext diffusers 0.31.0 transformer_flux.py], Qwen2-VL
 * q/k/v/o/gate/up/down [ext vLLM fork].  K % 64 == 0, N % 8 == 0; bias/gate/res may be NULL; res may
 * alias y.  Rounding points follow the reference's bf16 pipeline: Linear output, activation, gate
 * multiply and residual add each round to bf16.  act = TD_ACT_ID_* (other codes: TD_ERR_INVALID). */
int td_linear_bf16(const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy,
                   int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr,
                   void* stream);

/* Same contraction with two outputs: columns [0,n_split) -> y0 (act0), columns [n_split,N) -> y1
 * (act1).  This is FluxSingleTransformerBlock's fused [to_q|to_k|to_v|proj_mlp] projection
 * ([ext] transformer_flux.py FluxSingleTransformerBlock.forward).  n_split must be a multiple of the N tile the launcher
 * picks for the shape (64, 192 or 256 columns; 256 always qualifies -- TD_ERR_INVALID otherwise). */
int td_linear_split_bf16(const void* x, int64_t ldx, const void* w, const void* bias,
                         void* y0, int64_t ldy0, int act0, void* y1, int64_t ldy1, int act1,
                         int M, int N, int K, int n_split, void* stream);

/* y = x . w^T (+ bias) (+ res) with the contraction SPLIT over workgroups: few output tiles against a long K -- the KV-cached decode of 65..256
 * sequences (vLLM's max_num_seqs = 256, configs/qwen2_vl_embed_ccsbu.yaml:20: M <= 256 rows against N = hidden columns) -- would leave most CUs
 * idle.  split_k = -1: the launcher picks the parts (1 = an ordinary launch when a split does not pay), > 1: that many (must divide K / 64);
 * the parts' fp32 sums are added in index order by a second launch, so the result does not depend on scheduling.  y1 != NULL: columns >= n_split
 * go to y1 (n_split % 8 == 0).  M > 64 (smaller M is the weight-stream kernel's, which splits K itself).  tile_cfg as td_linear_grouped2_bf16
 * (4 = 256x128).  norm_w != NULL (split_k = -1, no y1, N % 512 == 0, N <= 4096): the reduction launch also writes norm_out[M, ld_norm] =
 * Qwen2RMSNorm(y0; norm_w, norm_eps) of each finished row, bit-identical to td_norm_rows_bf16 on y0 -- the decoder's o_proj -> post_attention_layernorm
 * and down_proj -> next input_layernorm pairs ([ext] transformers modeling_qwen2_vl.py Qwen2VLDecoderLayer.forward) as one Linear call. */
int td_linear_splitk_bf16(const void* x, int64_t ldx, const void* w, const void* bias, void* y0, int64_t ldy0, void* y1, int64_t ldy1, int n_split,
                          int M, int N, int K, const void* res, int64_t ldr, int tile_cfg, int split_k,
                          const void* norm_w, void* norm_out, int64_t ld_norm, float norm_eps, void* stream);

/* Two Linear problems in ONE launch (same N, K, strides, activation; own rows, weights, bias, gate,
 * residual): FluxTransformerBlock applies each projection to the image stream and to the text stream
 * with different weights ([ext] transformer_flux.py FluxTransformerBlock.forward: to_q/add_q_proj,
 * to_out/to_add_out, ff/ff_context); the 193-row text problem rides in the image problem's grid.
 * tile_cfg: -1 auto, 0 256x256, 1 256x64, 2 32x256, 3 288x192. */
int td_linear_grouped2_bf16(const void* x0, int M0, const void* w0, const void* bias0, const void* gate0,
                            const void* res0, void* y0, const void* x1, int M1, const void* w1,
                            const void* bias1, const void* gate1, const void* res1, void* y1,
                            int64_t ldx, int64_t ldy, int64_t ldr, int N, int K, int act, int tile_cfg,
                            void* stream);

/* Test entry of the 256x256 tile's persistent walk (td_abi_version() >= 9).  With several images in flight (td_flux_denoise_multi), a bf16 launch of
 * that tile with more tiles than CUs runs as one workgroup per CU, each walking tiles b, b + G, b + 2G, .. of the launch's tile order and storing
 * half of every tile's output from inside the next tile's main loop.  The environment variable TD_GEMM_DRAIN, read per launch, forces the
 * one-tile-per-workgroup launch (0) or the walk (1) everywhere.  Both forms give the same bits.
 * This entry is td_linear_grouped2_bf16 (x1 NULL: one problem) or, with y_split != NULL (one problem only), td_linear_split_bf16, always on the
 * 256x256 tile, with a bound on the number of walking workgroups: max_workgroups > 0 launches min(tiles, CUs, max_workgroups) of them, so that a
 * small problem walks several tiles per workgroup (max_workgroups >= tiles: the one-tile-per-workgroup launch); 0 = no bound. */
int td_linear_drain_bf16(const void* x0, int M0, const void* w0, const void* bias0, const void* gate0, const void* res0, void* y0,
                         const void* x1, int M1, const void* w1, const void* bias1, const void* gate1, const void* res1, void* y1,
                         int64_t ldx, int64_t ldy, int64_t ldr, int N, int K, int act,
                         void* y_split, int64_t ld_split, int act_split, int n_split, int max_workgroups, void* stream);

/* Which tile an automatic launch (tile_cfg = -1) of an M x N x K Linear takes (td_abi_version() >= 19): 0 256x256, 1 256x64, 2 32x256, 3 288x192.
 * Host arithmetic only: no device is touched, no stream is needed.  M = the rows of the launch (both problems of a grouped one), K in elements of
 * the operand type.  shared = 0: the launch has the chip to itself, and tiles are chosen by rounds of the CUs (the 288x192 tile where 256x256 leaves
 * one ragged round and K is long).  shared != 0: several images in flight (td_flux_denoise_multi) -- other images' kernels fill the CUs a launch
 * leaves empty, so the tile that costs the least CU time is taken, from a table of measured tile times per operand type.  operand: 0 bf16, 1 int8,
 * 2 e4m3 (-1, with td_last_error set, for anything else or for M, N, K < 1).  The environment variable TD_GEMM_SHARED_TILES, read per call and per
 * launch, forces the shared = 0 rule (0) or the CU-time choice (1) for every operand type under the hint.  Every tile gives the same bits. */
int td_gemm_plan_query(int M, int N, int K, int shared, int operand);

/* 3x3 convolution, stride 1, zero padding 1, over an NHWC bf16 image as an implicit GEMM (no im2col buffer):
 *   y[H*W, Cout] = conv3x3(x[Hin*Win, Cin]) + bias (+ res[H*W, Cout]);   upsample2x != 0 fuses the nearest 2x
 * upsample that precedes the conv in Upsample2D (then Hin = H/2, Win = W/2), else Hin = H, Win = W.
 * w is [Cout, 9*Cin] with k = (ky*3 + kx)*Cin + c (td_conv3x3_pack_weight converts from torch's [Cout,Cin,3,3]).
 * Cin % 64 == 0, Cout % 8 == 0.  Replaces nn.Conv2d(3x3) of [ext] diffusers AutoencoderKL.decode
 * (ResnetBlock2D.conv1/conv2, Upsample2D.conv, Decoder.conv_in/conv_out). */
int td_conv3x3_nhwc_bf16(const void* x, const void* w, const void* bias, const void* res, void* y,
                         int H, int W, int Cin, int Cout, int upsample2x, void* stream);
/* [Cout, Cin, 3, 3] (torch) -> [Cout_pad, 9*Cin_pad] (k = tap*Cin_pad + c), zero filled padding. */
int td_conv3x3_pack_weight(const void* w_oihw, void* w_packed, int Cout, int Cin, int Cout_pad, int Cin_pad, void* stream);
/* The two launches at the ends of td_vae_decode, alone (td_abi_version() >= 26; test entries: the engine runs the same kernels on its own buffers).
 * td_vae_latents_to_nhwc_bf16: packed FLUX latents [(h/2)(w/2), 4C] bf16 -> NHWC [h*w, Cpad] bf16, the statement
 * `(unpack_latents(packed) / scaling_factor) + shift_factor` on bf16 tensors ([ext] diffusers pipeline_flux.py): the quotient by the fp32 divisor
 * rounds to bf16, then the sum with bf16(shift_factor) rounds; channels C .. Cpad-1 are zero.  h, w even, Cpad >= C, no null pointer.
 * td_vae_image_finalize: x [P, Cpad] bf16 NHWC, its first three channels -> image_u8 [P, 3] = round(clamp(x / 2 + 0.5, 0, 1) * 255) with the
 * quotient, the sum and the clamp in bf16 and the product in fp32 ([ext] diffusers VaeImageProcessor.postprocess), and / or image_chw [3, P] bf16,
 * the same bits transposed.  Either output may be NULL, not both; Cpad >= 3; channels >= 3 of x are never read. */
int td_vae_latents_to_nhwc_bf16(const void* packed, void* out, int C, int h, int w, int Cpad, float scaling_factor, float shift_factor, void* stream);
int td_vae_image_finalize(const void* x, int P, int Cpad, void* image_u8, void* image_chw, void* stream);
/* y[M,N] (fp32) = x[M,K] . w[N,K]^T (+ bias): unrounded rows, e.g. attention scores. */
int td_linear_f32out_bf16(const void* x, int64_t ldx, const void* w, const void* bias, float* y, int64_t ldy,
                          int M, int N, int K, void* stream);

/* o[b,s,h*128+d] = softmax(q.k^T * scale (+causal mask)) . v, head_dim 128, fp32 softmax state.
 * q/k/v/o are token-major: row s of batch b at  ptr + b*bstride + s*ld  (elements), head h at
 * column h*128, so the fused QKV projection output is consumed in place.  Hq % Hkv == 0 (GQA).
 * causal != 0: key j visible to query i iff j <= i + (Skv - Sq).
 * Replaces F.scaled_dot_product_attention in [ext] diffusers 0.31.0 attention_processor.py
 * FluxAttnProcessor2_0 / FluxSingleAttnProcessor2_0 (joint [text||image] attention, no mask) and
 * the vLLM fork's Qwen2-VL attention (thinkdiff/models/mllama_vllm_t5_embed_decoder_2.py:1083). */
int td_attention_bf16(const void* q, int64_t ldq, int64_t q_bstride, const void* k, const void* v,
                      int64_t ldkv, int64_t kv_bstride, void* o, int64_t ldo, int64_t o_bstride,
                      int batch, int Sq, int Skv, int Hq, int Hkv, int head_dim, float scale,
                      int causal, void* stream);
/* Packed variable-length form (the vision towers' cu_seqlens, [ext] Qwen2VisionTransformerPretrainedModel.forward: full attention
 * inside each image / frame): q, k, v, o are [total rows, ld] with segment b = rows [seg_starts[b], seg_starts[b+1]); seg_starts is a
 * DEVICE int32[n_seg + 1]; max_len = the longest segment (sizes the grid).  One launch for all segments, no mask across them. */
int td_attention_varlen_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo,
                             const int* seg_starts, int n_seg, int max_len, int Hq, int Hkv, float scale, void* stream);
/* The packed form with a causal switch (td_abi_version() >= 17).  causal = 1: query row i of a segment sees the segment's rows j <= i -- the launch of
 * the Qwen2-VL engine's packed prefill (td_qwen2_prefill_packed: prompts back to back, no padding rows), parameters filled as the engine fills them.
 * causal = 0: td_attention_varlen_bf16 bit for bit.  max_len may exceed the longest segment (it only sizes the grid); max_len = 1 (every segment
 * one row) runs the same kernel.  TD_ERR_INVALID before any HIP call for: an empty segment list, a null operand, causal outside {0, 1},
 * Hq % Hkv != 0, a row stride shorter than its heads, ldq or ldkv not a multiple of 8 elements (16 bytes), ldo not a multiple of 4 (8 bytes),
 * q / k / v / o not 16-byte aligned, seg_starts not 4-byte aligned. */
int td_attention_segments_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo,
                               const int* seg_starts, int n_seg, int max_len, int Hq, int Hkv, float scale, int causal, void* stream);
/* Context attention (td_abi_version() >= 23): the packed causal form over key ranges of their own -- prompts continued behind cached prefixes, what vLLM
 * calls context attention.  Segment b owns q / o rows [seg_starts[b], seg_starts[b+1]) (Sq_b rows); its keys are rows [kv_row0[b], kv_row0[b] + kv_lens[b])
 * of k / v, counted in rows of ldkv (a KV cache seen as rows: kv_row0[b] = slot x slot rows).  Query row i of the segment sees keys
 * 0 .. kv_lens[b] - Sq_b + i: the last Sq_b keys are the segment's own tokens, the ones in front its prefix.  seg_starts int32[n_seg + 1], kv_row0 and
 * kv_lens int32[n_seg], all DEVICE arrays.  max_q_len >= the longest query segment (it sizes the grid), max_kv_len >= the longest key range (it sizes the
 * 4 GiB range check); either may exceed the longest.  The buffer descriptors cover the segment's own keys only, so rows of a neighbouring slot are never
 * read; kv_lens[b] < Sq_b counts as Sq_b.  With every prefix empty and k / v the packed rows this is td_attention_segments_bf16(causal = 1).
 * TD_ERR_INVALID before any HIP call for: an empty segment list, kv_row0 or kv_lens null, max_kv_len < max_q_len, a null operand, Hq % Hkv != 0, a row
 * stride shorter than its heads, ldq or ldkv not a multiple of 8 elements, ldo not a multiple of 4, q / k / v / o not 16-byte aligned, an int array not
 * 4-byte aligned. */
int td_attention_prefix_segments_bf16(const void* q, const void* k, const void* v, void* o, int64_t ldq, int64_t ldkv, int64_t ldo, const int* seg_starts,
                                      const int* kv_row0, const int* kv_lens, int n_seg, int max_q_len, int max_kv_len, int Hq, int Hkv, float scale, void* stream);
/* The joint attention in the form the FLUX engine calls it: q already carries scale x log2(e) (folded in where RoPE rounds q to bf16), so the
 * scores arrive in the exp2 domain; one batch entry, Hq == Hkv = H, head_dim 128.  score_bound in (0, 48]: a bound of |q'.k| (log2 units) the
 * caller vouches for -- the scores are then exponentiated as they are: no reference point, no per-tile row maximum, no rescale (a bf16 probability
 * keeps its mantissa at any magnitude and the sums are fp32: exp2(+-48) is far inside the range).  FLUX has such a bound by construction: the
 * QK-RMSNorm leaves |q'| <= premul x sqrt(128) x max|w_q| and |k| <= sqrt(128) x max|w_k|.  A score a few octaves past the bound is harmless.
 * 0: the running-maximum form (any scores).  Replaces F.scaled_dot_product_attention inside
 * [ext] diffusers FluxAttnProcessor2_0 (after norm_q / norm_k and apply_rotary_emb). */
int td_attention_joint_prescaled_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo, int S, int H,
                                      float score_bound, void* stream);
/* The joint (unmasked, one batch entry, Hq == Hkv) attention with BOTH products on the block-scaled e4m3 matrix instruction
 * (csrc/attention_fp8.hip): the same bf16 q / k / v / o and strides as td_attention_bf16; q, k, v are packed to e4m3 under
 * power-of-two scales (q, k per (token, head); v per (64-key tile, head)) in one pass into `workspace`
 * (td_attention_fp8_workspace_bytes(Sq, Skv, Hq) bytes, 16-byte aligned, contents undefined afterwards), the probabilities
 * are rounded to e4m3, accumulation and the softmax state stay fp32.  An option of the 8-bit modes (the reference graph has no
 * such path): its error is ~5 % of an attention output on random operands, see DESIGN.md section 4 for what it does to an image. */
size_t td_attention_fp8_workspace_bytes(int Sq, int Skv, int Hq);
int td_attention_fp8(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo,
                     int Sq, int Skv, int Hq, float scale, void* workspace, void* stream);
/* The same attention fed from the RAW fused projection buffer: the pack pass applies the per-head QK-RMSNorm (weights may be NULL) and the
 * interleaved-pair rotary embedding of td_qk_norm_rope_bf16(rotate_half = 0) on its way to e4m3 -- bit-identical to calling that kernel
 * and then td_attention_fp8, minus one HBM round trip over q | k; qkv is left unmodified.  Replaces, in the 8-bit attention mode, [ext] diffusers FluxAttnProcessor2_0: attn.norm_q / norm_k (+ norm_added_*) ->
 * apply_rotary_emb -> F.scaled_dot_product_attention.  qkv [S, ld] bf16 with q / k / v head blocks at columns q_col / k_col / v_col; cos,
 * sin fp32 [S,128]; rows < split take (wqA, wkA), the rest (wqB, wkB). */
int td_attention_fp8_qk_rope(const void* qkv, int64_t ld, int q_col, int k_col, int v_col, void* o, int64_t ldo, int S, int H,
                             const float* cos, const float* sin, int split, const void* wqA, const void* wkA, const void* wqB, const void* wkB,
                             float eps, float scale, void* workspace, void* stream);
/* Selects the kernel structure td_attention_bf16 launches: 0 = shipped (joint attention with more (query tile, head) items
 * than CUs runs as one round of persistent workgroups over equal KV-tile ranges; the first such call on a device allocates a
 * 35 MB hand-off workspace, so make it before capturing into a hipGraph), 1 = one workgroup per item for every shape, 2 = the
 * persistent form without the XCD-aware range order.  1 and 2 exist for in-process A/B measurements.  Returns the previous value. */
int td_attention_set_variant(int variant);
/* KV-cached decode attention (Sq = 1): q heads of one kv head handled per workgroup.  0 = automatic (the largest divisor of
 * Hq / Hkv among 7, 6, 4, 3, 2 that still gives every CU a workgroup, else 1); a divisor forces it (tests, A/B).  Returns the
 * previous value. */
int td_attention_decode_set_group(int g);

/* ---- row kernels (each is also used inside the FLUX engine) -------------------------------------- */

/* y = norm(x) [* w] [modulated]:  rms=0 LayerNorm(no affine, eps) as in [ext] diffusers
 * AdaLayerNormZero/Single/Continuous, rms=1 RMSNorm as T5LayerNorm (aligner tail,
 * thinkdiff/models/blip_vision_t5_decoder.py:50-53) and Qwen2RMSNorm.  Optional adaLN modulation
 * y = y*(1+scale)+shift with separate (shift,scale) for rows < split and rows >= split. D % 512 == 0. */
int td_norm_rows_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int rows, int D, int rms, float eps,
                      const void* w, int split, const void* shiftA, const void* scaleA,
                      const void* shiftB, const void* scaleB, void* stream);

/* In-place per-head RMSNorm(q), RMSNorm(k) (weights may be NULL = no norm) + rotary embedding on a
 * fused projection buffer.  rotate_half=0: FLUX interleaved pairs ([ext] diffusers apply_rotary_emb);
 * rotate_half=1: Qwen2 half-split (element i with i +- 64), y = bf16(x*cos + rotate_half(x)*sin) as one fp32 expression;
 * rotate_half=2: the same rotation with every op of the bf16 torch graph rounding, y = bf16(bf16(x*cos) + bf16(rotate_half(x)*sin))
 * (what the Qwen2-VL engine runs: bit-identical to transformers' apply_multimodal_rotary_pos_emb on bf16 tensors).
 * Any other rotate_half: TD_ERR_INVALID, nothing launched.  cos/sin: fp32 [rows,128]. */
int td_qk_norm_rope_bf16(void* qkv, int64_t ld, int rows, int Hq, int Hk, int q_col, int k_col,
                         const float* cos, const float* sin, int split, const void* wqA, const void* wkA,
                         const void* wqB, const void* wkB, float eps, int rotate_half, void* stream);

/* td_qk_norm_rope_bf16 with the factor the FLUX engine folds into q (td_abi_version() >= 25): q, not k, is multiplied by q_premul in fp32 behind the
 * rotation and in front of its one rounding to bf16 -- the engine passes attention scale * log2(e), so that the attention kernel needs no per-score
 * multiply.  q_premul = 1 gives td_qk_norm_rope_bf16's bits. */
int td_qk_norm_rope_premul_bf16(void* qkv, int64_t ld, int rows, int Hq, int Hk, int q_col, int k_col,
                                const float* cos, const float* sin, int split, const void* wqA, const void* wkA,
                                const void* wqB, const void* wkB, float eps, int rotate_half, float q_premul, void* stream);
/* The FLUX engine's conditioning vector (td_abi_version() >= 25; [ext] diffusers CombinedTimestepGuidanceTextProjEmbeddings.forward, then the nn.SiLU
 * in front of every AdaLayerNorm*'s Linear):  temb[r, c] = bf16(bf16(te[r, c] + ge[c]) + pe[c]);  silu_out[r, c] = bf16(silu(temb[r, c])).
 * te, temb, silu_out bf16 [n, D] contiguous; ge, pe bf16 [D].  ge NULL: temb = bf16(te + pe) (no guidance embedding).  temb NULL: only silu_out is
 * written.  te, pe or silu_out NULL, n <= 0 or D <= 0: TD_ERR_INVALID, nothing launched. */
int td_temb_combine_silu_bf16(const void* te, const void* ge, const void* pe, int n, int D, void* temb, void* silu_out, void* stream);
/* dst[r, 0 .. cols) = src[r, 0 .. cols) between two bf16 matrices of row strides lds, ldd (td_abi_version() >= 25; the channel-conditioned engine's
 * gather of the latents into cat(latents, cond)).  cols, lds, ldd multiples of 8, cols <= lds and cols <= ldd, both pointers 16-byte aligned; columns
 * of dst beyond cols are untouched.  Anything else: TD_ERR_INVALID, nothing launched. */
int td_copy_cols_bf16(const void* src, int64_t lds, void* dst, int64_t ldd, int rows, int cols, void* stream);

/* FluxPosEmbed tables: ids fp32 [S,3] -> cos,sin fp32 [S,128]. */
int td_flux_rope_table(const float* ids, int S, const int* axes_dims3, double theta, float* cos, float* sin, void* stream);
/* Timesteps(256) sinusoid: t fp32 [n] (device) -> bf16 [n,256] = [cos | sin]. */
int td_timestep_sincos(const float* t, int n, void* out, void* stream);
/* FlowMatchEulerDiscreteScheduler.step on bf16 latents: x = bf16(float(x) + dt*float(v)), product and sum each rounded
 * to fp32 as torch's `sample + dt * model_output` does (no fused multiply-add). */
int td_euler_step_bf16(void* x, const void* v, float dt, int64_t n, void* stream);
/* FluxInpaintPipeline's step: scheduler.step, scale_noise of the image latents to the next sigma, and the mask blend, fused, in
 * place on x; every op a bf16 torch op ([ext] pipeline_flux_inpaint.py, scheduling_flow_match_euler_discrete.py):
 *   a  = bf16(float(x) + float(bf16(bf16(dt) * float(v))))                          (td_euler_step_bf16's arithmetic)
 *   s  = bf16(sigma_next)
 *   p  = noise ? bf16(bf16(s * noise) + bf16(bf16(1 - s) * image_latents)) : image_latents
 *   x  = bf16(bf16(bf16(1 - mask) * p) + bf16(mask * a))
 * All operands bf16 [n], 16-byte aligned; n % 8 == 0; noise may be NULL (the loop's last step). */
int td_flux_inpaint_step_bf16(void* x, const void* v, const void* image_latents, const void* noise, const void* mask, float dt,
                              float sigma_next, int64_t n, void* stream);
/* FluxKontextPipeline's step under true classifier-free guidance, fused, in place on x ([ext] diffusers >= 0.34 pipeline_flux_kontext.py
 *   `noise_pred = neg_noise_pred + true_cfg_scale * (noise_pred - neg_noise_pred)`, then scheduler.step), every op a bf16 torch op;
 * `scale` is a Python float there, which eager torch keeps in fp32 as the operand of the bf16 multiply (it is not rounded to bf16 first):
 *   d = bf16(v_pos - v_neg);  m = bf16(scale * float(d));  v = bf16(v_neg + m);  x = bf16(float(x) + float(bf16(bf16(dt) * float(v))))
 * All operands bf16 [n], 16-byte aligned, n % 8 == 0, v_pos / v_neg not overlapping x. */
int td_flux_cfg_step_bf16(void* x, const void* v_pos, const void* v_neg, float scale, float dt, int64_t n, void* stream);
/* FLUX ControlNet residual injection, in place on h ([ext] diffusers >= 0.30 controlnet_flux.py `sample * conditioning_scale`, transformer_flux.py
 * `hidden_states = hidden_states + controlnet_block_samples[...]`), every op a bf16 torch op; `scale` is a Python float there, an fp32 operand of the
 * bf16 multiply as in td_flux_cfg_step_bf16:
 *   h[m, j] = bf16(float(h[m, j]) + float(bf16(scale * float(r[m, j]))))        m < rows, j < D
 * h, r bf16 with row strides ldh, ldr >= D (elements; columns beyond D are untouched); D % 8 == 0, strides multiples of 8, both pointers 16-byte
 * aligned, r not overlapping h. */
int td_flux_residual_inject_bf16(void* h, int64_t ldh, const void* r, int64_t ldr, int rows, int D, float scale, void* stream);
/* The same for n ControlNets at once (td_abi_version() >= 10; [ext] diffusers controlnet_flux.py FluxMultiControlNetModel.forward: the scaled samples
 * of the nets are summed in bf16 first, in list order, then the sum is added to hidden_states):
 *   s_k = bf16(scales[k] * float(r[k][m, j]));   acc = s_0;   acc = bf16(float(acc) + float(s_k))  for k = 1 .. n-1 (left fold, one rounding per add)
 *   h[m, j] = bf16(float(h[m, j]) + float(acc))                                  m < rows, j < D
 * -- not what n calls of td_flux_residual_inject_bf16 give, and one pass over h instead of n.  r, ldr, scales: HOST arrays of n entries
 * (1 <= n <= TD_MAX_CONTROLNETS), read during the call and passed to the kernel by value (no device-side table: capturable).  Checked before the
 * launch, TD_ERR_INVALID naming k: every r[k] non-null, 16-byte aligned, ldr[k] a multiple of 8 and >= D, not overlapping h; every scales[k] finite
 * (a NaN or infinite scale is refused, as td_flux_set_controlnet_scales refuses it).  n == 1 gives td_flux_residual_inject_bf16's bits. */
#define TD_MAX_CONTROLNETS 4
int td_flux_residual_inject_multi_bf16(void* h, int64_t ldh, const void* const* r, const int64_t* ldr, const float* scales, int n, int rows, int D,
                                       void* stream);
/* First-block cache kernels (td_abi_version() >= 6; what the engine's cache runs, td_flux_set_block_cache below).  bf16 rows of D columns (D % 8 == 0)
 * at row strides that are multiples of 8 and at least D, every pointer 16-byte aligned.
 * td_block_cache_head_bf16:   r[m, j] = bf16(float(h1[m, j]) - float(h0[m, j]))
 *                             sums[0] = sum |float(r) - float(r_prev)|,   sums[1] = sum |float(r_prev)|      over all rows x D elements, fp64 (device)
 * r_prev NULL = no previous residual: r is written, sums[0] = sums[1] = 0.  r overlaps none of the inputs.  The sums are taken without atomics in one
 * combination order fixed by (rows, D) -- fp32 per thread over at most a few dozen terms, fp64 above -- so the same inputs give the same bits on every
 * run, whatever else the device runs.  ws: TD_BLOCK_CACHE_WS_BYTES of device scratch, not shared by launches that may run concurrently.
 * td_block_cache_tail_bf16:   out[m, j] = bf16(float(a[m, j]) - float(b[m, j]));  out may be a or b (same stride): in place. */
#define TD_BLOCK_CACHE_WS_BYTES 65536
int td_block_cache_head_bf16(const void* h1, int64_t ld1, const void* h0, int64_t ld0, const void* r_prev, int64_t ldp, void* r, int64_t ldr, int rows, int D,
                             double* sums, void* ws, void* stream);
int td_block_cache_tail_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int rows, int D, void* stream);
/* FLUX.1 Redux prompt composition (td_abi_version() >= 8; [ext] diffusers FluxPriorReduxPipeline.__call__, restated from the published source, parity
 * unpinned): B [text | image] prompt streams, each under its own scale, summed into ONE stream of T + S rows -- the pipeline's
 *   prompt_embeds = cat([text, image_embeds], dim=1);  prompt_embeds *= scale[:, None, None];  prompt_embeds = sum(prompt_embeds, dim=0)
 * on bf16 tensors, without the concatenated intermediate.  out [T + S, ldo] bf16:
 *   out[r, :D]     = bf16( sum_{b = 0 .. B-1} float( bf16( s_b * text[b, r, :] ) ) )          r < T
 *   out[T + r, :D] = bf16( sum_{b = 0 .. B-1} float( bf16( s_b * image[b, r, :] ) ) )         r < S
 * Rounding: s_b = scales[b] rounded to bf16 (on the host, by this entry); each product rounded to bf16; the sum in fp32 in index order b = 0, 1, ..,
 * starting from the b = 0 term, rounded once (B = 1 with scale 1 returns the inputs' bits).  Source rows are contiguous (D elements apart), batch
 * entries text_bstride / image_bstride elements apart.  text NULL = zero rows: +0.0 is written, nothing read.  text_bstride 0 = one text stream shared
 * by every b, still added B times, each under its scale (one string prompt with several images).  Columns D .. ldo-1 of out are not written.  T == 0 or
 * S == 0 is allowed, not both (the pooled vector: T = 1, S = 0, D = 768).  scales: B floats in HOST memory, read before the launch; they travel in
 * the kernel's argument segment.  out overlaps neither input.
 * TD_ERR_INVALID, nothing launched: D % 8 != 0; B < 1 or B > 16; T < 0, S < 0, T + S == 0; ldo < D or ldo % 8 != 0; image NULL with S > 0; scales NULL;
 * out NULL; a batch stride negative or not a multiple of 8; a pointer not 16-byte aligned; (T + S) x D > INT32_MAX elements (32-bit index). */
int td_redux_compose_bf16(const void* text, int64_t text_bstride, int T, const void* image, int64_t image_bstride, int S,
                          const float* scales /* host, B floats */, int B, int D, void* out, int64_t ldo, void* stream);
/* FLUX IP-Adapter cross-attention (td_abi_version() >= 5; [ext] diffusers >= 0.32 FluxIPAdapterJointAttnProcessor2_0, restated from the published
 * source, parity unpinned): the image rows' query against the n_keys image-prompt tokens of one adapter, the scaled result written or added to o.
 *   qn[m, h, :] = norm_w ? bf16(bf16(q[m, h, :] * rstd) * norm_w)  :  q[m, h, :]       rstd = rsqrt(mean(q[m, h, :]^2) + eps) in fp32 (qk_norm8 of
 *                 csrc/qk_rope_math.h with td_qk_norm_rope_bf16's summation tree: the bits that kernel rounds before it rotates)
 *   s[m, h, j]  = sum_d qn[m, h, d] k[j, h*128 + d]                  fp32 accumulation of bf16 products (v_mfma_f32_16x16x32_bf16), j < n_keys
 *   p[m, h, j]  = bf16(exp2((s - max_j s) * 128^-0.5 * log2(e)))     the TRUE row maximum over all n_keys (k is not normalised: no score bound)
 *   a[m, h, d]  = bf16((sum_j p[m, h, j] v[j, h*128 + d]) / (sum_j p[m, h, j]))      fp32 accumulation; the row sum is over the rounded p
 *   t           = bf16(out_scale * float(a))                         `scale` is a Python float in diffusers: an fp32 operand of a bf16 multiply
 *   o[m, h*128 + d] = accumulate ? bf16(float(o[m, h*128 + d]) + float(t)) : t
 * q bf16 [rows, ldq] with head h at column h*128 (the FLUX engine passes the image rows of its [S, 3D] projection buffer, ldq = 3D); k, v bf16
 * [n_keys, ldkv]; o bf16 [rows, ldo]; norm_w bf16 [128] or NULL.  rows >= 1, 1 <= H <= 65535, 1 <= n_keys <= TD_IP_MAX_KEYS; strides multiples of 8
 * and >= H*128; all pointers 16-byte aligned.  Keys are scored in tiles of 32: the kernel zero-fills the padding in LDS and masks its scores, and
 * reads nothing outside [n_keys, ldkv].  Columns of o beyond H*128 and rows beyond `rows` are untouched.  Anything else: TD_ERR_INVALID before any
 * launch, the offender named.  Capturable (no allocation, no synchronisation). */
#define TD_IP_MAX_KEYS 256       /* two images of a 128-token adapter */
int td_ip_attention_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo, int rows, int H, int n_keys,
                         const void* norm_w, float eps, float out_scale, int accumulate, void* stream);
#define TD_INPAINT_MASK_U8_HW 0   /* uint8 [H, W] (PIL mode "L") */
#define TD_INPAINT_MASK_F32_HW 1  /* float32 [H, W] in [0, 1] */
/* FluxInpaintPipeline's mask latents from a height x width mask (format TD_INPAINT_MASK_*):
 *   m = binarize(mask)          (uint8: u8 / 255 >= 0.5, i.e. u8 >= 128; float32: v >= 0.5)
 *   m = F.interpolate(m, (H/8, W/8), nearest)      (the exact factor 8: latent pixel (y, x) takes m[8y, 8x])
 *   packed_out = _pack_latents(m.repeat(1, C, 1, 1))   -> bf16 [(H/16)(W/16), 4C] of 0 / 1
 * H, W multiples of 16; C even; packed_out 16-byte aligned. */
int td_flux_inpaint_mask(const void* mask, int format, int H, int W, int C, void* packed_out, void* stream);
/* FLUX.1 Fill's channel condition of one image, in one pass ([ext] diffusers >= 0.32 pipeline_flux_fill.py prepare_mask_latents):
 * cond_out bf16 [S, 4C + 256], S = (H/16)(W/16), h = H/8, w = W/8:
 *   columns 0 .. 4C-1:       _pack_latents((latent_dist.sample(eps) - shift) * scaling) of the MASKED image's moments [h*w, 2C]
 *                            (td_vae_encode_masked) -- td_vae_latents_from_moments with noise = NULL, its arithmetic and rounding points;
 *                            eps bf16 [C, h, w], NULL = .mode()
 *   columns 4C .. 4C+255:    the binarized mask (td_flux_inpaint_mask's rule) at FULL resolution, unshuffled, not sampled:
 *                            mask[H, W].view(h, 8, w, 8).permute(1, 3, 0, 2).reshape(64, h, w) -> _pack_latents, i.e. column
 *                            4C + (py*8 + px)*4 + dy*2 + dx of token (Y, X) = m[8(2Y + dy) + py, 8(2X + dx) + px] as bf16 0 / 1.
 * H, W multiples of 16; C even; cond_out 16-byte aligned. */
int td_flux_fill_condition(const void* moments, const void* eps, const void* mask, int mask_format, int H, int W, float scaling_factor,
                           float shift_factor, int C, void* cond_out, void* stream);
/* FluxPipeline._pack_latents (unpack=0: [C,H,W] -> [(H/2)(W/2),4C]) / _unpack_latents (unpack=1, with
 * out = bf16(bf16(in / div) + add), i.e. the `latents / scaling_factor + shift_factor` on bf16 tensors that precedes
 * vae.decode in [ext] pipeline_flux.py, with torch's CPU scalar rules: fp32 divisor, addend cast to bf16, quotient and sum
 * each round to bf16; div = 1, add = 0 is a pure unpack). */
int td_flux_pack_latents(const void* src, void* dst, int C, int H, int W, int unpack, float div, float add, void* stream);
/* ThinkDiff-CLIP token pooling (blip_vision_t5_decoder.py:620-637): [1+G*G,C] -> [1+(G/2)^2,C]. */
int td_cls_avgpool2_bf16(const void* x, void* y, int G, int C, void* stream);
/* counter-based N(mean,std) fill (synthetic checkpoints for throughput runs). */
int td_fill_normal_bf16(void* dst, int64_t n, uint64_t seed, float std, float mean, void* stream);
/* ... of a piece of a larger buffer (td_abi_version() >= 25): element i of dst draws what element 2 * pair0 + i of td_fill_normal_bf16 with the same seed
 * draws.  Elements come in pairs: pair p = splitmix64(seed + 0x9E3779B97F4A7C15 * (p + 1)) gives u1 from its top 24 bits and u2 from the next 24, and
 * Box-Muller in fp32 gives elements 2p (cosine) and 2p + 1 (sine).  pair0 < 0: TD_ERR_INVALID, nothing launched. */
int td_fill_normal_from_bf16(void* dst, int64_t n, uint64_t seed, float std, float mean, int64_t pair0, void* stream);

/* ThinkDiff aligner `mm_projector` of type "mlp2x_gelu_t5_norm" (every shipped config):
 *   y = T5LayerNorm(Linear2(GELU_erf(Linear0(x))))        x:[M,K] -> y:[M,hidden]
 * Replaces build_vision_projector's nn.Sequential (thinkdiff/models/blip_vision_t5_decoder.py:31-61,
 * call sites :641 and thinkdiff/models/mllama_vllm_t5_embed_decoder_2.py:1113-1116).  State-dict
 * tensors: w0 = mm_projector.0.weight [hidden,K], b0, w2 = mm_projector.2.weight [hidden,hidden], b2,
 * norm_w = mm_projector.3.weight [hidden].  workspace: 2*M*hidden bf16.  K % 64 == 0, hidden % 512 == 0.
 * fp32_norm != 0 reproduces the LVLM path (fp32 norm params under autocast: no bf16 rounding inside
 * the norm, output rounded once). */
int td_aligner_mlp2x_bf16(const void* x, int64_t ldx, int M, int K, int hidden, const void* w0, const void* b0,
                          const void* w2, const void* b2, const void* norm_w, float eps, int fp32_norm,
                          void* workspace, void* y, int64_t ldy, void* stream);

/* ---- FLUX.1 MMDiT denoise engine ------------------------------------------------------------------
 * Replaces the `diffusion_pipe(prompt_embeds=..., pooled_prompt_embeds=..., height, width,
 * num_inference_steps, guidance_scale)` denoise loop the reference drivers call
 * (scripts/test/test_blip_vision_t5_decoder_flux_text.py:234-242, scripts/test/
 * test_mllama_t5_decoder_flux.py:182-192), i.e. [ext] diffusers 0.31.0 FluxTransformer2DModel.forward
 * + FlowMatchEulerDiscreteScheduler.step.  Parameters are addressed by their diffusers state-dict
 * names (e.g. "transformer_blocks.3.attn.to_k.weight"), so a FLUX.1-dev checkpoint loads unchanged. */
typedef struct td_flux td_flux;
typedef struct TdFluxConfig {
  int in_channels;        /* 64  */
  int num_layers;         /* 19  */
  int num_single_layers;  /* 38  */
  int num_heads;          /* 24  */
  int head_dim;           /* 128 */
  int joint_dim;          /* 4096 */
  int pooled_dim;         /* 768 */
  int guidance_embeds;    /* 1   */
  int mlp_ratio;          /* 4   */
  int axes_dims[3];       /* 16,56,56 */
  float rope_theta;       /* 10000 */
  int out_channels;       /* 0 = in_channels (FLUX.1-dev: 64).  FLUX.1 Fill 64 of 384, FLUX.1 Canny / Depth 64 of 128: the checkpoints whose
                           * x_embedder reads the latents and a per-image condition concatenated along the channel axis, in_channels =
                           * out_channels + C_cond, while proj_out, the velocity and the latents the scheduler steps keep out_channels.
                           * Both multiples of 64.  Last field: a caller that zero-fills the struct keeps the unconditioned model. */
} TdFluxConfig;

/* max_img_tokens bounds the IMAGE STREAM of a forward: the latents' tokens plus the reference tokens of td_flux_set_reference_tokens, if any. */
int td_flux_create(const TdFluxConfig* cfg, int max_img_tokens, int max_txt_tokens, int max_steps, td_flux** out);
void td_flux_destroy(td_flux* f);
int64_t td_flux_param_elems(const td_flux* f);
int td_flux_num_params(const td_flux* f);
int td_flux_param_info(const td_flux* f, int idx, char* name_buf, int buf_len, int64_t* count);
/* copy one parameter (device bf16, `count` elements) into the engine's fused weight arena.  TD_ERR_INVALID while the parameter holds a LoRA
 * base copy (td_flux_lora_load): clear the adapters first.  td_flux_init_random likewise. */
int td_flux_load_param(td_flux* f, const char* name, const void* src, int64_t count, void* stream);
/* A second context over the same weights (own workspace, conditioning, timestep schedule): independent images in flight on
 * separate streams fill the tails of each other's kernels (a 1024^2 step's grids are 1.6 - 3.2 rounds of the 256 CUs).
 * The parent must outlive its forks; parameters and precision are the parent's.  Destroy with td_flux_destroy. */
int td_flux_fork(td_flux* parent, td_flux** out);
/* td_flux_denoise for `count` contexts (a parent and its forks), advanced step by step, context k on streams[k]. */
int td_flux_denoise_multi(td_flux* const* fs, void* const* latents, int count, const float* sigmas, int n, void* const* streams);
/* td_flux_denoise_multi with the inpainting step of td_flux_denoise_inpaint: image_latents[k], noise[k], mask[k] blend context k. */
int td_flux_denoise_multi_inpaint(td_flux* const* fs, void* const* latents, int count, const float* sigmas, int n,
                                  const void* const* image_latents, const void* const* noise, const void* const* mask, void* const* streams);

/* Operand precision of the block GEMMs.  TD_PRECISION_FP8_E4M3 quantises every double-/single-stream Linear weight per
 * output channel from the parameters as loaded NOW (call after loading; call again after reloading) and runs those GEMMs on
 * the fp8 MFMA path with per-token dynamic activation scales (BASELINE config 5).  Accumulation, epilogues, attention,
 * normalisation and the residual stream stay as in the bf16 path. */
enum { TD_PRECISION_BF16 = 0, TD_PRECISION_FP8_E4M3 = 1,
       /* W8A8 symmetric int8 (round 3): the same per-output-channel weight / per-token activation scaling and the same 2x-bf16 MFMA
        * rate (v_mfma_i32_16x16x64_i8, exact int32 accumulation), with a uniform step of max/127 instead of e4m3's 3-bit mantissa */
       TD_PRECISION_INT8 = 2 };
int td_flux_set_precision(td_flux* f, int precision, void* stream);
/* TD_PRECISION_INT8 only: source of the per-token activation scales of the MLP operands.  0 (default) = measured on the spot (one
 * quantisation pass per tensor); 1 = the maxima the PREVIOUS denoise step accumulated for the same tensor and token x 1.25 (clip beyond):
 * the MLP intermediate then leaves the producing GEMM epilogue as int8.  First steps and out-of-order steps use mode 0.  Parent context. */
int td_flux_set_act_scales(td_flux* f, int mode);
/* TD_PRECISION_INT8 only: per-channel smoothing of the activations that carry outlier channels (SmoothQuant's balance at alpha = 1/2, factors
 * rounded to powers of two so that x / s and W s are exact).  mode 1: the FIRST int8 forward after the mode, the precision or a parameter changed
 * runs on the bf16 path and records per-channel maxima of the LayerNorm outputs and MLP intermediates; from then on those activations are divided by
 * s[channel] where they are quantised (LayerNorm kernel, int8 GEMM epilogue, quantisation pass) and the consuming weights' input channels are
 * multiplied by s before their own quantisation.  Per-token int8 then no longer spends its 8 bits on a few channels that run tens of times above
 * the rest (the failure mode of W8A8 on trained DiTs; tests/test_flux_full_depth_gpu.py grades it on the heavy-tailed fixture).  0 = off (default).
 * The reference has no such path (it runs bf16): this belongs to BASELINE config 5's 8-bit MFMA path.  Parent context. */
int td_flux_set_smoothing(td_flux* f, int mode);
/* Arithmetic of the joint attention in every block: TD_ATTENTION_BF16 (default: the reference graph's) or TD_ATTENTION_FP8 (QK^T and P.V
 * on the e4m3 matrix instruction, td_attention_fp8).  Independent of td_flux_set_precision; meant for the 8-bit modes.  Parent context. */
enum { TD_ATTENTION_BF16 = 0, TD_ATTENTION_FP8 = 1 };
int td_flux_set_attention(td_flux* f, int mode);
/* Which block Linears take the fp8 path while the precision is TD_PRECISION_FP8_E4M3 (default: all).  The rest run in bf16 from
 * the bf16 weights: a speed / deviation-from-bf16 trade.  Parent context only; takes effect at the next step. */
enum { TD_FP8_QKV = 1, TD_FP8_OUT = 2, TD_FP8_FF1 = 4, TD_FP8_FF2 = 8,      /* double-stream blocks: to_q|k|v (+add_*), to_out, ff.net.0, ff.net.2 */
       TD_FP8_SINGLE_IN = 16, TD_FP8_SINGLE_OUT = 32,                        /* single-stream blocks: to_q|k|v + proj_mlp, proj_out */
       TD_FP8_ALL_GEMMS = 63 };
int td_flux_set_fp8_gemms(td_flux* f, unsigned mask);
int td_flux_init_random(td_flux* f, uint64_t seed, float std, void* stream);
/* per prompt: prompt_embeds bf16 [T,joint_dim], pooled bf16 [pooled_dim], ids fp32 device [n,3]
 * (txt_ids NULL = zeros, thinkdiff/models/flux_prompt.py:119).  Always voids the context's reference tokens (it rebuilds the RoPE table for
 * T + S_img rows): set them again after it, for every image; a forward without them is the plain model. */
int td_flux_set_condition(td_flux* f, const void* prompt_embeds, int T, const void* pooled, const float* txt_ids,
                          const float* img_ids, int S_img, void* stream);
/* per schedule: t_eff (host, n floats) / g_eff = the values fed to the sinusoids (timestep*1000,
 * guidance*1000 after the pipeline's dtype casts); precomputes temb and every adaLN modulation */
int td_flux_set_timesteps(td_flux* f, const float* t_eff, int n, float g_eff, void* stream);
/* The extents a prepared context expects: image / text tokens of the last td_flux_set_condition (0 before it), latent channels, prepared
 * timesteps.  Any out pointer may be NULL.  (The torch.ops layer checks tensor extents against it before handing pointers over.)
 * `in_channels` is the width of the LATENTS and of the velocity (TdFluxConfig::out_channels; on an unconditioned engine that is also
 * x_embedder's width -- td_flux_input_shape reports the two apart). */
int td_flux_prepared_shape(const td_flux* f, int* img_tokens, int* txt_tokens, int* in_channels, int* n_steps);
/* What x_embedder reads: its width (TdFluxConfig::in_channels), the channel condition's share of it (in_channels - out_channels, 0 on an
 * unconditioned engine) and whether this context holds a valid channel condition.  Any out pointer may be NULL. */
int td_flux_input_shape(const td_flux* f, int* in_channels, int* cond_channels, int* cond_valid);
/* The per-image channel condition of a conditioned engine (C_cond = in_channels - out_channels > 0): cond bf16 [S_img, C_cond], S_img of the
 * last td_flux_set_condition, 16-byte aligned; copied into this context's x_embedder staging rows at columns out_channels .. in_channels - 1
 * (forks own theirs), where every later forward of the image finds it.  Replaces the `torch.cat([latents, masked_image_latents], dim=2)` /
 * `torch.cat([latents, control_image], dim=2)` that [ext] diffusers >= 0.32 FluxFillPipeline / FluxControlPipeline.__call__ make in front of
 * every transformer call.  td_flux_set_condition with another S_img invalidates it; a forward without a valid one is TD_ERR_INVALID (never
 * a run on zeros); on an unconditioned engine the call itself is TD_ERR_INVALID.  Forgets the 8-bit modes' per-token history like
 * td_flux_set_condition (another image). */
int td_flux_set_channel_condition(td_flux* f, const void* cond, void* stream);
/* FLUX.1 Kontext's reference tokens of one image: ref_latents bf16 [S_ref, out_channels] (packed, already shifted / scaled, 16-byte aligned),
 * ref_ids device fp32 [S_ref, 3].  After td_flux_set_condition, once per image, this context's own (forks hold theirs).  From then on every
 * forward of the context runs its blocks over [text | latents | reference] -- T + S_img + S_ref rows, the reference rows with the RoPE
 * of ref_ids -- while the final AdaLayerNorm, proj_out, the velocity and every step kernel keep the S_img latent rows.  Replaces, in
 * [ext] diffusers >= 0.34 FluxKontextPipeline.__call__, `latent_model_input = torch.cat([latents, image_latents], dim=1)`,
 * `latent_ids = torch.cat([latent_ids, image_ids], dim=0)` and `noise_pred = noise_pred[:, : latents.size(1)]` of every step.
 * S_ref == 0 (null pointers allowed) clears.  TD_ERR_INVALID: no condition set; S_img + S_ref > max_img_tokens; a channel-conditioned
 * engine; misaligned pointers.  Forgets the 8-bit modes' per-token history like td_flux_set_condition (another image). */
int td_flux_set_reference_tokens(td_flux* f, const void* ref_latents, int S_ref, const float* ref_ids, void* stream);
/* The reference tokens this context holds (0: none, or no condition set). */
int td_flux_reference_tokens(const td_flux* f, int* S_ref);
/* velocity[S_img,out_channels] = transformer(latents[S_img,out_channels]; prepared step).  On a conditioned engine the latents are gathered
 * beside the channel condition and x_embedder runs as ONE Linear over in_channels, as on torch.cat([latents, cond]). */
int td_flux_forward(td_flux* f, const void* latents, int step, void* velocity, void* stream);
/* ---- FLUX ControlNet (td_abi_version() >= 4): a side network of the same double- / single-stream blocks with its own weights
 * ([ext] diffusers >= 0.30 FluxControlNetModel: InstantX FLUX.1-dev-Controlnet-Canny / -Union, Shakker Union-Pro).  TdFluxConfig describes it as it
 * describes a transformer (num_layers = n_d >= 1, num_single_layers = n_s >= 0, guidance_embeds as the checkpoint has it, out_channels 0); the
 * struct itself is unchanged, the kind and num_mode travel as arguments.  Parameters: the transformer's without norm_out / proj_out, plus
 * controlnet_x_embedder, controlnet_blocks.{i}, controlnet_single_blocks.{i} (weight + bias) and, with num_mode > 0 ("union" checkpoints),
 * controlnet_mode_embedder.weight [num_mode, D].  The handle is a td_flux: parameters, td_flux_fork, td_flux_set_condition, td_flux_set_timesteps
 * and td_flux_destroy are the transformer's.  It runs in bf16 only: td_flux_set_precision / td_flux_set_attention to an 8-bit mode and
 * td_flux_lora_load are TD_ERR_INVALID on it (the main transformer may be in any mode); td_flux_forward on it is TD_ERR_INVALID. */
int td_flux_controlnet_create(const TdFluxConfig* cfg, int num_mode, int max_img_tokens, int max_txt_tokens, int max_steps, td_flux** out);
/* Union models: the control mode, before td_flux_set_condition -- which then prepends controlnet_mode_embedder[mode] to the embedded prompt and
 * duplicates the first txt id (T + 1 text rows; td_flux_prepared_shape reports them) and is TD_ERR_INVALID with none set.  -1 clears.  Per context. */
int td_flux_controlnet_set_mode(td_flux* cn, int mode);
/* The control image of one image: control_latents bf16 [S_img, in_channels] (VAE latents, shifted / scaled, packed), 16-byte aligned, after
 * td_flux_set_condition.  Computes E = controlnet_x_embedder(control_latents) once; every forward adds it to x_embedder(latents) (each Linear's
 * output rounds to bf16, then the sum).  td_flux_set_condition with another S_img invalidates it. */
int td_flux_controlnet_set_condition(td_flux* cn, const void* control_latents, void* stream);
/* One ControlNet evaluation at a prepared step: behind block i the i-th output Linear writes controlnet_blocks[i](image stream) /
 * controlnet_single_blocks[i](image rows) into the context's sample arena, UNSCALED. */
int td_flux_controlnet_forward(td_flux* cn, const void* latents, int step, void* stream);
/* The sample arena of the last forward: sample k (double-block samples first, n_double + n_single in all) is bf16 [rows, width] contiguous at
 * base + k * stride_elems.  Any out pointer may be NULL. */
int td_flux_controlnet_samples(const td_flux* cn, void** base, int* n_double, int* n_single, int64_t* stride_elems, int* rows, int* width);
/* Copy sample k of the last forward into dst, bf16 [rows, width] contiguous (stream-ordered). */
int td_flux_controlnet_read_sample(const td_flux* cn, int k, void* dst, void* stream);
/* Attach ONE ControlNet context to a main context (NULL detaches); a ControlNet context serves one main context at a time (forks pair up: one
 * ControlNet fork per main context).  From then on td_flux_forward -- and with it every td_flux_denoise* loop -- at a step whose scale is not 0
 * first runs the ControlNet on the same latents, step and stream, then adds   bf16(scale * sample[i / ceil(n_blocks / n_samples)])   to the image
 * rows behind double block i, and likewise behind single block i (td_flux_residual_inject_bf16; trailing samples the index never reaches are
 * unused; n_s = 0: no single-block injection).  A step with scale 0, and a context with nothing attached, issue the plain forward's launches.
 * Forward-time TD_ERR_INVALID: inner width, heads or latent width differ; the ControlNet context is prepared for another S_img or step count, or
 * holds no control condition; reference tokens are set; the main engine is channel-conditioned.  Attaching resets the scales to 1.0. */
int td_flux_attach_controlnet(td_flux* f, td_flux* cn);
/* conditioning scale per prepared step (n host floats; steps beyond n keep 1.0): controlnet_conditioning_scale x controlnet_keep[i]. */
int td_flux_set_controlnet_scales(td_flux* f, const float* scales, int n);
/* ---- Several ControlNets on one main context (td_abi_version() >= 10; [ext] diffusers FluxMultiControlNetModel, restated from the published
 * controlnet_flux.py / pipeline_flux_controlnet.py, parity unpinned).  td_flux_attach_controlnets attaches cns[0 .. n) in list order, 0 <= n <=
 * TD_MAX_CONTROLNETS; n = 0 detaches all.  td_flux_attach_controlnet(f, cn) is its n = 1 form, cn == NULL its n = 0 form.  Every context obeys the
 * one-main-context rule above; the same context listed twice is TD_ERR_INVALID (two appearances of one MODEL are two forks).  Attaching resets
 * every net's scale table to 1.0; a refused call changes nothing.
 * td_flux_forward at a step: the nets whose scale at the step is not 0 are the ACTIVE ones.  Each passes the forward-time checks above (messages
 * name k), then they run one after another on the same latents, step and stream, and behind each block ONE td_flux_residual_inject_multi_bf16
 * launch over the active nets in list order adds   bf16(h + fold_k bf16(scale_k * sample_k[idx_k]))   to the image rows.
 * Deviations from diffusers, both deliberate: (1) every net uses ITS OWN index rule idx_k = i / ceil(n_blocks / n_samples_k) (diffusers zips the
 * nets' sample lists and silently truncates when the counts differ; with equal counts the two agree), and a net with n_s = 0 takes no part in the
 * single-block sums; (2) a net whose scale at the step is 0 is not run and is left out of the fold (diffusers adds bf16(0 * x): at most the sign of
 * a zero differs).  A step at which every scale is 0, and a context with nothing attached, issue exactly the plain forward's launches. */
int td_flux_attach_controlnets(td_flux* f, td_flux* const* cns, int n);
/* Net k's conditioning scale per prepared step (as td_flux_set_controlnet_scales, which is k = 0); k outside the attached count is TD_ERR_INVALID. */
int td_flux_set_controlnet_scales_at(td_flux* f, int k, const float* scales, int n);
/* The attached count (0 .. TD_MAX_CONTROLNETS). */
int td_flux_attached_controlnets(const td_flux* f, int* n);
/* ---- FLUX IP-Adapter (td_abi_version() >= 5): image-prompt conditioning of the double-stream blocks ([ext] diffusers >= 0.32 FluxIPAdapterMixin,
 * embeddings.ImageProjection, attention_processor.FluxIPAdapterJointAttnProcessor2_0, transformer_flux.FluxTransformerBlock.forward; restated from
 * the published sources, parity unpinned).  Up to TD_IP_MAX_ADAPTERS adapters in numbered slots.  Per adapter, J = joint_dim, D = heads x 128:
 *   tokens = LayerNorm_J(Linear(embeds [n_img, E] -> [n_img, num_tokens J]).reshape(n_img num_tokens, J))     eps 1e-5, affine; once per image
 *   K_i = to_k_ip_i(tokens), V_i = to_v_ip_i(tokens)      Linear(J -> D, bias), double block i; once per image, not per step
 * and in double block i, for the adapters in slot order:   ip = 0;  ip += scale_a[i] * SDPA(norm_q(to_q(norm_hidden)), K_i^a, V_i^a)   -- the image
 * stream's query BEFORE RoPE, every op a bf16 torch op (td_ip_attention_bf16 spells the roundings) -- then, behind `hidden + gate_mlp * ff`,
 *   hidden = bf16(float(hidden) + float(ip))      (td_flux_residual_inject_bf16 at scale 1.0, which is exact).
 * ip is neither projected by to_out nor gated; the text stream and the single-stream blocks are untouched.  The adapter's weights stay bf16 in every
 * precision mode, to_q runs in whatever mode the model is in, and nothing of it joins the int8 smoothing calibration or the history scales.
 *
 * Model level -- parent context only (forks share the model, as with LoRA); TD_ERR_INVALID on a fork and on a ControlNet.
 * td_flux_ip_adapter_add: claims the first free slot for an adapter of num_tokens tokens per image over embeddings of width embed_dim (% 8 == 0)
 * and allocates its weights (not capturable, like td_flux_lora_load).  Parameter names of td_flux_ip_adapter_load_param (device bf16, `count`
 * elements, torch Linear layout): image_proj.proj.weight [num_tokens J, E], image_proj.proj.bias, image_proj.norm.weight [J], image_proj.norm.bias,
 * ip_adapter.{i}.to_k_ip.weight [D, J], ip_adapter.{i}.to_k_ip.bias [D], ip_adapter.{i}.to_v_ip.weight, ip_adapter.{i}.to_v_ip.bias, i < num_layers.
 * td_flux_ip_adapter_remove frees a slot (-1: all).  td_flux_set_ip_adapter_scale: n == 1 (all blocks) or n == num_layers finite host floats;
 * default 1.0; a block whose scale is 0 contributes nothing and launches nothing. */
#define TD_IP_MAX_ADAPTERS 4
int td_flux_ip_adapter_add(td_flux* f, int num_tokens, int embed_dim, int* slot);
int td_flux_ip_adapter_load_param(td_flux* f, int slot, const char* name, const void* data, int64_t count, void* stream);
int td_flux_ip_adapter_remove(td_flux* f, int slot);
int td_flux_set_ip_adapter_scale(td_flux* f, int slot, const float* per_block, int n);
/* Slot facts (any out pointer may be NULL): used, num_tokens, embed_dim; and on THIS context whether embeds are set and for how many keys. */
int td_flux_ip_adapter_info(const td_flux* f, int slot, int* used, int* num_tokens, int* embed_dim, int* embeds_set, int* n_keys);
/* Per context (forks hold their own image prompt): embeds bf16 [n_img, E] contiguous, 16-byte aligned; NULL clears the slot for this context.
 * Runs the projection (the engine's GEMM, td_layernorm_bf16) and the 2 x num_layers K / V Linears into this context's arena
 * [L][K | V][keys_pad][D], n_keys = n_img x num_tokens, rows up to the multiple of 32 zero.  Allocates at first use and when a later call needs more
 * (hipMalloc / hipFree: NOT capturable, like td_flux_lora_load).  TD_ERR_INVALID: a free slot, a parameter of the slot not loaded yet (named),
 * n_img x num_tokens > TD_IP_MAX_KEYS (both numbers in the message), a ControlNet context.
 * Forward-time TD_ERR_INVALID of a context with embeds set (td_flux_forward and every td_flux_denoise* loop): the slot's weights changed or the slot
 * was removed since (td_flux_ip_adapter_load_param / _remove: set the embeds again, or clear them); reference tokens are set (the image rows would
 * include the reference rows); a ControlNet is attached.  A context with no embeds set, or with every scale 0, issues the plain forward's launches
 * and gives its bits; one active slot adds two launches per double block (td_ip_attention_bf16, td_flux_residual_inject_bf16), each further one. */
int td_flux_set_ip_image_embeds(td_flux* f, int slot, const void* embeds, int n_img, void* stream);
/* Tests: copy this context's image-prompt tokens (block < 0: bf16 [n_keys, J]) or double block `block`'s K (which = 0) / V (1) (bf16 [n_keys, D])
 * of a slot into dst, contiguous, stream-ordered. */
int td_flux_ip_read(const td_flux* f, int slot, int block, int which, void* dst, void* stream);
/* The widths of those rows: J = joint_dim (tokens) and D = heads x 128 (K / V). */
int td_flux_ip_widths(const td_flux* f, int* joint_dim, int* inner_dim);
/* ---- First-block cache (td_abi_version() >= 6; [ext] diffusers >= 0.33 hooks/first_block_cache.py `FirstBlockCacheConfig`, restated from the
 * published source, parity unpinned): skip the transformer on forwards whose first block's output barely moved.  With the cache on, every
 * td_flux_forward -- and with it every td_flux_denoise* loop -- runs the embedders and double block 0 as always (an IP-Adapter's add included), then
 *   r      = bf16(float(h1) - float(h0))                       h0 / h1: the S_img + S_ref image rows before / behind the block
 *   metric = sum |r - r_prev| / sum |r_prev|                   r_prev: r of the last COMPUTED forward; sums as td_block_cache_head_bf16 takes them, the
 *                                                              ratio in double on the host (diffusers rounds both means and the ratio to bf16)
 * and is COMPUTED -- r_prev <- r, the remaining blocks run, tail = bf16(float(h_final) - float(h1)) is kept for the S_img latent rows -- when there
 * is no r_prev, when the mode's rule says so (mode 1: metric > threshold; mode 2: the schedule's entry for this forward, counted from the last reset,
 * 1 beyond its end), or when an int8 smoothing calibration is pending; otherwise SKIPPED: h = bf16(float(h1) + float(tail)) on the latent rows
 * (td_flux_residual_inject_bf16 at scale 1.0), then the final norm and proj_out as always.  A skipped forward leaves the context's 8-bit history as an
 * out-of-order step does: the next forward starts its history scales and softmax references afresh.  The decision needs the sums on the host: one
 * 16-byte copy and one synchronisation of the forward's stream per forward -- only with the cache on; mode 0 issues exactly the plain launches.
 * State (r_prev, tail, the log) is per context and reset by: every td_flux_denoise* loop at its start, a change of the token layout (T, S_img, S_ref),
 * of the model's weights (LoRA) or of these settings, and td_flux_block_cache_reset.  It is allocated at a context's first forward under the cache
 * (hipMalloc: not capturable).
 * Settings are the model's -- parent context only, forks follow.  td_flux_set_block_cache: mode 0 off, 1 threshold (>= 0; 0 = always compute).
 * td_flux_set_block_cache_schedule: mode 2, compute[i] != 0 = forward i is computed; compute[0] must be 1; the metric is still taken and logged.
 * TD_ERR_INVALID: a fork; a ControlNet model; a forward with the cache on and a ControlNet attached (its samples are added behind every block: that
 * pairing is not built); a negative or NaN threshold; a mode other than 0 / 1; a schedule that is empty or starts with 0; a model without a double block.
 * td_flux_block_cache_stats: the log since the last reset -- *n forwards, and for the first min(cap, *n) of them the metric (+inf where there was no
 * r_prev) and whether the forward was computed.  metric / computed may be NULL with cap 0. */
int td_flux_set_block_cache(td_flux* f, int mode, float threshold);
int td_flux_set_block_cache_schedule(td_flux* f, const unsigned char* compute, int n);
int td_flux_block_cache_reset(td_flux* f);
int td_flux_block_cache_stats(const td_flux* f, int cap, float* metric, unsigned char* computed, int* n);
/* Per-launch HIP-event trace of the engine's kernels (events recorded on the launch stream).
 * categories: 0 GEMM 256x256 tile (td_gemm_bf16_nt_kernel<8,4>), 1 small GEMM tiles, 2 attention,
 * 3 LayerNorm+modulate, 4 QK-RMSNorm+RoPE, 5 GEMM 288x192 tile (<9,3>).  trace_end synchronises and
 * fills 6-element arrays. */
int td_flux_trace_begin(td_flux* f, int max_launches);
int td_flux_trace_end(td_flux* f, void* stream, int64_t* counts, double* ms, double* flops);
/* n Euler steps in place; sigmas: n+1 host floats */
int td_flux_denoise(td_flux* f, void* latents, const float* sigmas, int n, void* stream);
/* FluxKontextPipeline's loop under true classifier-free guidance ([ext] diffusers >= 0.34 pipeline_flux_kontext.py, `do_true_cfg`): n steps
 * in place, each the transformer on `pos` and on `neg` (two prepared contexts -- in practice a context and its fork: shared weights, own
 * conditioning, own 8-bit history), then td_flux_cfg_step_bf16 with dt = sigmas[i+1] - sigmas[i].  ONE stream.  Reference tokens, if any, are
 * set on both contexts by the caller.  TD_ERR_INVALID: contexts whose S_img, S_ref, out_channels or prepared step count differ; pos == neg;
 * latents overlapping either context's velocity buffer. */
int td_flux_denoise_cfg(td_flux* pos, td_flux* neg, void* latents, const float* sigmas, int n, float scale, void* stream);
/* FluxInpaintPipeline's loop: n steps in place, each the transformer then td_flux_inpaint_step_bf16 with
 *   dt = sigmas[i+1] - sigmas[i],  sigma_next = sigmas[i+1],  noise used for i < n-1 (the last step blends the clean image_latents).
 * image_latents (the packed clean latents z), noise (the packed start noise) and mask (td_flux_inpaint_mask's output): bf16
 * [S_img, out_channels] (the latents' width), 16-byte aligned, none NULL, none overlapping the latents. */
int td_flux_denoise_inpaint(td_flux* f, void* latents, const float* sigmas, int n, const void* image_latents, const void* noise,
                            const void* mask, void* stream);

/* ---- LoRA adapters: low-rank weight merge --------------------------------------------------------------------------
 * On this engine an adapter is always MERGED: W_eff = W + sum_i weight_i * (alpha_i / rank_i) * B_i A_i, recomputed from an untouched copy of
 * the base weight with one rounding whenever the adapters or their weights change.  The forward afterwards is the code that exists (same kernels,
 * same launch count; the 8-bit modes quantise W_eff), and the merge is a pure function of (base, active adapters, weights): switching adapters
 * never drifts, unloading gives back the base bits.  Replaces [ext] peft LoraLayer.forward / merge / unmerge as [ext] diffusers
 * FluxLoraLoaderMixin drives them (load_lora_weights, set_adapters, fuse_lora / unfuse_lora, delete_adapters, unload_lora_weights).
 * The reference drivers load no LoRA: this belongs to the FLUX.1 pipelines' own surface. */
#define TD_LORA_MAX_ADAPTERS 8   /* active adapters on ONE parameter (one td_lora_merge_bf16 call) */
/* The kernel's operand form of one (lora_A.weight [rank, K], lora_B.weight [N, rank]) pair: A transposed [K, r_pad] then B [N, r_pad], the rank
 * zero-padded to r_pad = 16 ceil(rank / 16) (one k-step of the bf16 matrix instruction), so that every fragment is one 16-byte read.  Made once
 * per adapter, not per merge.  td_lora_packed_bytes: its size (0 for rank < 1 or empty extents). */
size_t td_lora_packed_bytes(int rank, int N, int K);
int td_lora_pack_bf16(const void* A, const void* B, int rank, int N, int K, void* packed, void* stream);
/* w_out[n, k] = RNE_bf16( float(w_base[n, k]) + sum_i scales[i] * sum_r B_i[n, r] A_i[r, k] ): peft's `weight + scaling * (B @ A)` for up to
 * TD_LORA_MAX_ADAPTERS pairs at once.  w_base, w_out bf16 [N, K] contiguous, 16-byte aligned, w_out may BE w_base (in place); packed[i] from
 * td_lora_pack_bf16 with the same N, K; any rank >= 1; K % 64 == 0, N % 8 == 0.  Inner products on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation; scales[i] multiplies the fp32 sum of adapter i; the base joins in fp32; one rounding.  Pairs with scale 0 are skipped, and with
 * none left w_out receives the base bits.  TD_ERR_INVALID before any launch for anything else. */
int td_lora_merge_bf16(const void* w_base, void* w_out, int N, int K, int n_adapters, const void* const* packed, const int* ranks,
                       const float* scales, void* stream);
/* ---- Row-indexed low-rank add (td_abi_version() >= 24; csrc/lora_rows.hip): the UNMERGED form, every row under an adapter of its own, behind a base
 * Linear that has already written y.  For a row whose adapter has A [r, K], B [N, r] and scale s:
 *   t_j = bf16_rne( sum_k x_k A_jk )                                 fp32 accumulation; products are exact
 *   y_n = bf16_rne( float(y_n) + s * sum_j float(t_j) B_nj )         fp32 accumulation; ONE rounding
 * Rows with row_adapter[row] = -1 (or outside 0 .. n_adapters - 1) are not written, nor are rows whose adapter has a null operand for the segment.  No
 * float atomics: K is split into slabs by a rule of K alone and the slabs are added in order, so a call is bit-reproducible and a row's result does not
 * depend on the rows beside it.  What vLLM's punica shrink / expand pair does behind `enable_lora` ([ext] vllm/lora/ops), restated.
 *   x            bf16 [rows, K], leading dimension ldx (>= K, % 8 == 0), 16-byte aligned; K % 64 == 0
 *   row_adapter  DEVICE int32 [rows], read by the kernels: a captured launch stays valid when the assignment changes
 *   packed       HOST array [n_adapters * n_segs] of device pointers, entry a * n_segs + s = the td_lora_rows_pack_bf16 form of adapter a's pair for
 *                segment s (N = widths[s], the same K), or NULL: adapter a does not touch segment s
 *   ranks/scales HOST [n_adapters]: rank 1 .. TD_LORA_ROWS_MAX_RANK, finite scale (looked at only for adapters with a non-null operand)
 *   y/ldy/widths HOST [n_segs], 1 .. TD_LORA_ROWS_MAX_SEGS output segments: device bf16 pointer (8-byte aligned), leading dimension (>= width, % 4 == 0),
 *                width (% 16 == 0).  A fused Linear is one call: [q | k | v] is three segments on one x, q into one buffer and k, v into another
 *   ws/ws_bytes  device workspace of at least td_lora_rows_workspace_bytes(rows, K, n_segs, largest rank) bytes, 16-byte aligned; nothing is allocated
 * TD_ERR_INVALID, naming the argument, before any HIP call for anything else.  With no non-null operand nothing is launched. */
#define TD_LORA_ROWS_MAX_SEGS 3
#define TD_LORA_ROWS_MAX_RANK 64
/* Ap [r_pad, K] = lora_A.weight, then Bp [N, r_pad] = lora_B.weight, the rank zero-padded to r_pad = 16 ceil(rank / 16); N % 16 == 0, K % 64 == 0 */
size_t td_lora_rows_packed_bytes(int rank, int N, int K);
int td_lora_rows_pack_bf16(const void* A, const void* B, int rank, int N, int K, void* packed, void* stream);
size_t td_lora_rows_workspace_bytes(int rows, int K, int n_segs, int max_rank);
int td_lora_rows_bf16(const void* x, int64_t ldx, int rows, int K, const int32_t* row_adapter, int n_adapters, const void* const* packed, const int* ranks,
                      const float* scales, int n_segs, void* const* y, const int64_t* ldy, const int* widths, void* ws, size_t ws_bytes, void* stream);
/* The parameter AS THE FORWARD SEES IT NOW (the effective weight: base + merged adapters) -> dst (device bf16, `count` elements): the inverse of
 * td_flux_load_param; what `transformer.state_dict()[name]` is after fuse_lora. */
int td_flux_read_param(td_flux* f, const char* name, void* dst, int64_t count, void* stream);
/* [N, K] of a Linear's `.weight` parameter, [count, 1] of a 1-D one (biases, norm scales).  The engine takes N, K of an adapter pair from here:
 * a C caller of td_flux_lora_load vouches that A holds rank x K and B N x rank elements (the torch.ops layer checks its tensors against it). */
int td_flux_param_shape(const td_flux* f, const char* name, int64_t* rows, int64_t* cols);
/* Attach one low-rank pair of adapter `adapter` to the `.weight` of one Linear (`param` = its diffusers state-dict name, e.g.
 * "transformer_blocks.3.attn.to_k.weight"): A = lora_A.weight [rank, K], B = lora_B.weight [N, rank], device bf16, 16-byte aligned;
 * scale = lora_alpha / rank.  Replaces peft's inject_adapter + set_peft_model_state_dict for that module.  Copies the pair into engine-owned
 * device memory in the kernel's operand form; the first pair on a parameter also takes the BASE COPY of it.  Allocates (like
 * td_flux_set_precision: not capturable).  Changes no weight yet: a new adapter is inactive until td_flux_lora_set_adapters names it.
 * TD_ERR_INVALID, naming the offender: a fork; an unknown, 1-D or non-`.weight` parameter; rank < 1; a non-finite scale; misaligned pointers;
 * a second pair for the same (adapter, parameter). */
int td_flux_lora_load(td_flux* f, const char* adapter, const char* param, const void* A, const void* B, int rank, float scale, void* stream);
/* diffusers' set_adapters(names, weights): the n named adapters become the active set with these weights, every other adapter inactive, and EVERY
 * parameter any loaded adapter touches is recomputed from its base copy with scales weights[i] * scale (one td_lora_merge_bf16 launch each);
 * n == 0: all inactive, base bits.  In an 8-bit precision the block weights are then quantised again from the merged ones (td_flux_set_precision's
 * pass) and the int8 history / smoothing calibration is forgotten as after td_flux_load_param.  Bumps the weight epoch: a context whose
 * td_flux_set_condition / td_flux_set_timesteps ran before it refuses td_flux_forward / td_flux_denoise* until both ran again (they precompute
 * the embedders and every adaLN modulation FROM weights).  The caller keeps merges off streams that run forwards on these weights.
 * TD_ERR_INVALID: a fork; an unknown or repeated adapter name; a non-finite weight; more than TD_LORA_MAX_ADAPTERS active on one parameter
 * (nothing is changed then). */
int td_flux_lora_set_adapters(td_flux* f, const char* const* names, const float* weights, int n, void* stream);
/* diffusers' delete_adapters(name) / unload_lora_weights(): drop one / all adapters and recompute what they touched; a parameter no adapter
 * touches any more gets its base bits back and its base copy is freed.  Synchronises the stream (memory is released).  Weight epoch as above. */
int td_flux_lora_delete(td_flux* f, const char* adapter, void* stream);
int td_flux_lora_clear(td_flux* f, void* stream);
/* Bookkeeping: loaded adapters, parameters holding a base copy, device bytes held (operands + base copies; with every Linear of FLUX.1-dev
 * targeted the base copies are one more weight arena).  Any out pointer may be NULL. */
int td_flux_lora_info(const td_flux* f, int* n_adapters, int* n_params_touched, int64_t* bytes_held);

/* ---- fp8 operand path (BASELINE config 5 "fp8 MFMA FLUX path") -------------------------------
 * Operands are OCP e4m3 bytes with one fp32 dequantisation scale per row: weights per output channel (quantised once at
 * load), activations per token (quantised by the kernel that produces them).  The contraction runs on
 * v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales) at twice the bf16 MFMA rate; everything after the
 * accumulators (bias, activation, gate, residual, bf16 rounding points) is the bf16 epilogue. */
/* q[r,:] = e4m3(x[r,:] / s_r), s_r = max|x[r,:]| / 448 (1 for an all-zero row) -> scale[r].  K % 8 == 0. */
int td_quant_rows_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int K, void* stream);
/* y = epilogue((xq . wq^T) * x_scale[m] * w_scale[n]); same epilogue arguments as td_linear_bf16.  K % 128 == 0. */
int td_linear_fp8(const void* xq, int64_t ldx, const float* x_scale, const void* wq, const float* w_scale, const void* bias,
                  void* y, int64_t ldy, int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr,
                  int tile_cfg, void* stream);
/* ---- int8 operand path (round 3; TD_PRECISION_INT8) -- the 8-bit form whose pixels stay inside the 1e-2 bar at full coverage -----
 * Same scaling scheme and call shape as the fp8 entries: q[r,:] = rint(x[r,:] / s_r) as int8, s_r = max|x[r,:]| / 127 (1 for an
 * all-zero row); the contraction runs on v_mfma_i32_16x16x64_i8 (exact int32 accumulation) at twice the bf16 MFMA rate. */
int td_quant_rows_int8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int K, void* stream);
int td_linear_int8(const void* xq, int64_t ldx, const float* x_scale, const void* wq, const float* w_scale, const void* bias,
                   void* y, int64_t ldy, int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr,
                   int tile_cfg, void* stream);
/* td_norm_rows_bf16 whose output row is quantised in registers: q [rows, ldq] e4m3 + q_scale[rows] (no bf16 copy). */
int td_norm_rows_quant_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* q_scale, int rows, int D, int rms, float eps,
                           const void* w, int split, const void* shiftA, const void* scaleA, const void* shiftB, const void* scaleB,
                           void* stream);

/* ---- int8 policy building blocks (td_abi_version() >= 7) -----------------------------------------------------------------------------------
 * The launch forms of the 8-bit policy that only the FLUX engine used to reach (int8 block Linears, history scales, per-channel smoothing with
 * replicated outlier channels, int8 attention output), one thin entry each, so that every kernel of the policy can be compared with its exact integer
 * statement (tests/test_int8_policy_gpu.py).  The reference graph has none of this (it runs bf16): it belongs to BASELINE config 5's 8-bit MFMA path.
 * The quantisation arithmetic, everywhere below, in fp32 and in this order:
 *     s = amax * (1.0f / 127)   (448 for e4m3; 1.0f where amax == 0)      inv = 1.0f / s      q = clamp(rint(v * inv), -127, 127)   (half to even)
 * Every entry refuses NULL required pointers, misaligned rows and extents that do not fit with TD_ERR_INVALID before any HIP call. */

/* td_norm_rows_bf16 whose output row y leaves quantised, with smoothing and replicated channels (all of td_norm_rows_bf16's arguments first):
 *   v[j]       = float(y[j]) * float(smooth[j])         smooth = smoothA for rows < split, smoothB for the others (bf16 [D]; NULL = none): a product
 *                                                       of two bf16 values, exact in fp32
 *   q_scale[r] = s(max_j |v[j]|),   q[r, j] = q(v[j])   j < D;   int8 != 0: symmetric int8, else OCP e4m3 under max / 448 (td_norm_rows_quant_fp8)
 *   q[r, D + e] = ext[e] >= 0 ? q[r, ext[e]] : 0        e < ext_n; ext = extA / extB by the same row split (device int32 [ext_n], entries < D);
 *                                                       int8 form only, both tables or none, ext_n even
 * q rows are ldq bytes apart, ldq % 8 == 0, ldq >= D + ext_n; bytes beyond D + ext_n are untouched. */
int td_norm_rows_quant8(const void* x, int64_t ldx, void* q, int64_t ldq, float* q_scale, int rows, int D, int rms, float eps,
                        const void* w, int split, const void* shiftA, const void* scaleA, const void* shiftB, const void* scaleB,
                        int int8, const void* smoothA, const void* smoothB, const int* extA, const int* extB, int ext_n, void* stream);
/* td_quant_rows_int8 (int8 != 0) / td_quant_rows_fp8 with per-column factors and the row maxima:
 *   v[r, j] = float(x[r, j]) * col_mul[j]  (fp32 [K], 16-byte aligned; NULL = none),   scale[r] = s(max_j |v[r, j]|),   q[r, j] = q(v[r, j]),
 *   amax_out[r] = the float bits of max_j |v[r, j]|  (NULL = not wanted).   K % 8 == 0; ldx (elements) and ldq (bytes) multiples of 8, >= K. */
int td_quant_rows8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int K, int int8, const float* col_mul, uint32_t* amax_out, void* stream);
/* amax[j] = max(amax[j], max_r |x[r, j]|) on float bits (all values >= 0: unsigned order is float order), j < K, r < rows; a column of zeros leaves
 * its accumulator as it was.  x bf16 [rows, ldx], K % 8 == 0. */
int td_col_amax_bf16(const void* x, int64_t ldx, int rows, int K, uint32_t* amax, void* stream);
/* SmoothQuant's balance at alpha = 1/2 rounded to a power of two, from two arrays of maxima (float bits, as td_col_amax_bf16 leaves them):
 *   s[i] = 2^clamp(rint(0.5 * (log2 amax_x[i] - log2 amax_w[i])), -8, 8)   (1 where either maximum is 0),   inv[i] = 1 / s[i],   inv_bf16[i] = bf16(inv[i]) */
int td_smooth_factors(const uint32_t* amax_x, const uint32_t* amax_w, int n, float* s, float* inv, void* inv_bf16, void* stream);
/* History scales: scale[i] = float(amax[i]) * margin * (1.0f / 127) in fp32, left to right (1.0f where amax[i] == 0), inv[i] = 1.0f / scale[i], and
 * amax[i] = 0 for the step being started.  margin >= 1 (the engine: 1.25). */
int td_q8_scales_from_amax(uint32_t* amax, float* scale, float* inv, int64_t n, float margin, void* stream);
/* q[r, K + e] = ext[e] >= 0 ? q[r, ext[e]] : 0   for e < ext_n, r < rows: the replicated input channels of an int8 weight whose rows are ld >= K + ext_n
 * bytes apart (ext: device int32 [ext_n], entries < K).  The K original bytes and the bytes beyond K + ext_n are untouched. */
int td_ext_cols_int8(void* q, int64_t ld, int rows, int K, const int* ext, int ext_n, void* stream);
/* td_linear_int8 whose activated result leaves as int8 under per-row scales fixed IN ADVANCE (the engine: last step's maxima x 1.25):
 *   t = bf16(acc * x_scale[m] * w_scale[n] + bias[n])        acc: the exact int32 contraction; the dequantisation in fp32
 *   a = bf16(act(t))                                          (act = TD_ACT_ID_NONE: a = t)
 *   v = float(a) * float(q8_smooth[n])                        bf16 [N] indexed by the ABSOLUTE output column (NULL = none): 1 / s of the next Linear
 *   q8[m, n] = clamp(rint(v * q8_inv[m]), -127, 127),    q8_amax[m] = max(q8_amax[m], max_n |v|)  on float bits
 * One problem of such a launch: */
typedef struct TdLinearQ8Problem {
  const void* xq; const float* x_scale;      /* int8 [M, ldx], fp32 [M] */
  const void* wq; const float* w_scale;      /* int8 [N, K] contiguous, fp32 [N] */
  const void* bias;                          /* bf16 [N] or NULL */
  void* q8;                                  /* int8 out [M, ldq8] (the int8 columns only, from column 0) */
  const float* q8_inv; uint32_t* q8_amax;    /* fp32 [M], float bits [M] */
  const void* q8_smooth;                     /* bf16 [N] or NULL */
  int M;
} TdLinearQ8Problem;
/* K % 128 == 0, N % 16 == 0, ldx and ldq8 multiples of 16, 16-byte aligned operands; tile_cfg 0 (256x256), 2 (32x256) or -1 (automatic; a shape for
 * which that picks the 288x192 tile is refused: it has no int8 output).  No bf16 output is written.  Bytes beyond N of a q8 row are untouched. */
int td_linear_int8_q8(const TdLinearQ8Problem* a, int64_t ldx, int64_t ldq8, int N, int K, int act, int tile_cfg, void* stream);
/* The split-output form (td_linear_split_bf16 on int8 operands): columns [0, n_split) -> y0 bf16 under act0 as td_linear_int8 writes them, columns
 * [n_split, N) -> a->q8[m, n - n_split] as int8 under act1, with q8_smooth still indexed by the absolute column n.  n_split % 256 == 0. */
int td_linear_split_int8_q8(const TdLinearQ8Problem* a, int64_t ldx, int64_t ldq8, void* y0, int64_t ldy0, int act0, int act1, int N, int K, int n_split, int tile_cfg,
                            void* stream);
/* Two problems in one launch (td_linear_grouped2_bf16 on int8 operands: same N, K, strides, activation; own rows, weights, scales, smoothing). */
int td_linear_grouped2_int8_q8(const TdLinearQ8Problem* a0, const TdLinearQ8Problem* a1, int64_t ldx, int64_t ldq8, int N, int K, int act, int tile_cfg, void* stream);
/* The joint attention (one batch entry, Hq == Hkv = H, head_dim 128) whose output leaves as int8: with o = the bf16 output td_attention_bf16 (plain
 * form, q_prescaled = 0) or td_attention_joint_prescaled_bf16 (q_prescaled != 0, score_bound as there; `scale` is then unused) writes for the same operands,
 *   q8[s, h*128 + d] = clamp(rint(float(o[s, h*128 + d]) * q8_inv[s]), -127, 127),    q8_amax[s] = max(q8_amax[s], max over all heads |o[s, :]|).
 * q8 rows are ldq8 bytes apart (% 8 == 0, >= H*128): the FLUX single-stream block passes its [attn | mlp] row, whose bytes beyond H*128 stay untouched.
 * causal / bias exist so that the call shape is td_attention_bias_bf16's: a non-zero causal or a non-NULL bias is TD_ERR_INVALID. */
int td_attention_q8(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* q8, int64_t ldq8, const float* q8_inv, uint32_t* q8_amax,
                    int Sq, int Skv, int H, float scale, int causal, const float* bias, int q_prescaled, float score_bound, void* stream);
/* The same over td_attention_fp8's output (same operands, workspace and arithmetic up to the store). */
int td_attention_fp8_q8(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* q8, int64_t ldq8, const float* q8_inv, uint32_t* q8_amax,
                        int Sq, int Skv, int H, float scale, void* workspace, void* stream);

/* ---- building blocks of the text encoders (T5-XXL, CLIP-L) feeding encode_prompt
 * (thinkdiff/models/flux_prompt.py:88-104 -> [ext] FluxPipeline._get_t5_prompt_embeds / _get_clip_prompt_embeds) ---- */
/* y = norm(x) for any D % 8 == 0: rms = 0 nn.LayerNorm(w, b, eps), rms = 1 T5LayerNorm(w). */
int td_layernorm_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int rows, int D, int rms, float eps,
                      const void* w, const void* b, void* stream);
/* out[r,:] = a[r,:] + b[r % b_rows,:]  (token + position embeddings, bias rows). */
int td_add_rows_bf16(const void* a, const void* b, void* out, int rows, int D, int b_rows, void* stream);
/* out[m,j] = act(gu[m,j]) * gu[m,I+j]  (T5 gated-GELU / SwiGLU); act = any TD_ACT_ID_* (other codes: TD_ERR_INVALID). */
int td_glu_mul_bf16(const void* gate_up, void* out, int rows, int I, int act, void* stream);
/* td_attention_bf16 with an additive fp32 score bias [Hq,Sq,Skv] (T5 relative position bias), batch 1. */
int td_attention_bias_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo,
                           int Sq, int Skv, int Hq, int Hkv, float scale, int causal, const float* bias, void* stream);

/* ---- building blocks of the vision towers upstream of the aligner (EVA-ViT-g = Blip2VisionModel,
 * thinkdiff/models/blip_vision_t5_decoder.py:611-618; Qwen2-VL ViT inside the vLLM engine,
 * thinkdiff/models/mllama_vllm_t5_embed_decoder_2.py:1083-1089) ---- */
/* In-place rotate_half RoPE over the first hd columns of H heads spaced head_stride apart; cos/sin fp32 [S, hd/2]. */
int td_rope_half_bf16(void* x, int64_t ldx, int S, int H, int head_stride, int hd, const float* cos_t, const float* sin_t, void* stream);
/* cos/sin fp32 [S, hd/2] of the 2-D vision rotary from pos int32 [S,2] = (row, column) of each patch (device). */
int td_vision_rope_table(const int* pos, int S, int hd, float theta, float* cos_t, float* sin_t, void* stream);
/* Conv2d(kernel = stride = p) operand: pix [C,H,W] (fp32 if src_f32 else bf16) -> out [(H/p)(W/p), Kpad] bf16, zero padded.  H / p and W / p round
 * down: the trailing H % p rows and W % p columns are dropped, as the convolution drops them (SigLIP so400m: 384 = 27 x 14 + 6). */
int td_patchify_bf16(const void* pix, int src_f32, int C, int H, int W, int p, void* out, int Kpad, void* stream);
/* Qwen2-VL image preprocessing after the resize ([ext] transformers Qwen2VLImageProcessor rescale / normalize / patchify, which
 * vLLM runs on the host for thinkdiff/models/mllama_vllm_generate_1.py:543-583): img uint8 [H,W,3] (device) -> out bf16
 * [(H/patch)(W/patch), Kpad] in the processor's merge-window row order, columns (c, t, py, px); lut fp32 [3,256] = the
 * processor's own rescale + normalize of every pixel value per channel (device). */
int td_qwen2_patchify_u8(const void* img_hwc, int H, int W, const float* lut, int patch, int merge, int temporal, void* out, int Kpad, void* stream);
/* ---- PIL-exact image resize ([ext] Pillow src/libImaging/Resample.c, the `Image.resize` every image processor upstream of the towers calls) ----
 * One axis' coefficient table, made on the HOST (no HIP call, no allocation: it runs on a machine without a GPU).  filter takes Pillow's own integer
 * codes, so a processor's `resample` passes straight through: 1 = LANCZOS (support 3), 2 = BILINEAR (support 1), 3 = BICUBIC (a = -0.5, support 2);
 * 0 (NEAREST), 4 (BOX), 5 (HAMMING) and anything else are TD_ERR_INVALID.  Arithmetic, in double, is Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc: scale = in / out, fs = max(scale, 1), support = filter_support * fs, ksize = ceil(support) * 2 + 1; per output xx:
 * center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), count = min((int)(center + support + 0.5), in) - xmin,
 * w[x] = filter((x + xmin - center + 0.5) * (1 / fs)), summed in index order and each divided by the sum, then (int)(+-0.5 + w * 2^22) with the sign
 * of w.  lanczos' sinc is sin(pi x) / (pi x) with libm's sin, which is why the table is not made in a kernel.
 * Fills bounds[out_size][2] = (xmin, count), kk[out_size][ksize] (rows zero past count) and *ksize; with bounds == kk == NULL only *ksize (query). */
int td_resize_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk, int* ksize);
/* src uint8 [in_h, in_w, in_c] -> dst uint8 [out_h, out_w, out_c] (device, contiguous) in Pillow's order: horizontal pass into tmp (uint8
 * [in_h, out_w, out_c], device), then vertical pass; each pass accumulates pixel * weight in int32 from 1 << 21 and writes clip8(acc >> 22).  A pass
 * whose size does not change is skipped (its table may be NULL); with both unchanged the call is a copy or the channel conversion alone; tmp is needed
 * only when both run.  h_* / v_* are the DEVICE copies of td_resize_coeffs' output for (in_w, out_w) / (in_h, out_h); the caller orders their upload
 * before this call on `stream`.  Channel forms, fixed by what Pillow's convert("RGB") does (the conversion happens in the first pass that runs):
 * 3 -> 3 RGB, 1 -> 1 "L", 1 -> 3 "L" replicated, 4 -> 3 "RGBA" with alpha dropped; every other pair is TD_ERR_INVALID.  No allocation, no
 * synchronisation; every refusal (non-positive sizes, bad channel pair, missing table or tmp, element counts past 2^31) comes before any launch. */
int td_image_resize_u8(const void* src_hwc, int in_h, int in_w, int in_c, void* dst_hwc, int out_h, int out_w, int out_c, const int32_t* h_bounds, const int32_t* h_kk,
                       int h_ksize, const int32_t* v_bounds, const int32_t* v_kk, int v_ksize, void* tmp, void* stream);
/* out fp32 [C, H, W] = lut[c][img[y, x, c]] for img uint8 [H, W, C], lut fp32 [C, 256] (device): a processor's rescale + normalize of every pixel value
 * per channel, computed by the processor's own arithmetic on the host, so the result is the host path's bit for bit.  1 <= C <= 4. */
int td_image_lut_chw_f32(const void* img_hwc, int H, int W, int C, const float* lut, float* out, void* stream);
/* out[r, :K] = bf16(src[r, :K]); out[r, K:Kpad] = 0. */
int td_cast_pad_rows_bf16(const void* src, int src_f32, int rows, int K, void* out, int Kpad, void* stream);

/* ---- FLUX VAE decoder (AutoencoderKL.decode) -------------------------------------------------------------
 * Replaces the tail of the drivers' `diffusion_pipe(...)` call: [ext] diffusers 0.31.0 FluxPipeline
 * `_unpack_latents` + `latents / scaling_factor + shift_factor` + `vae.decode` + `image_processor.postprocess`
 * (scripts/test/test_blip_vision_t5_decoder_flux_text.py:234-247).  Parameters use the diffusers names
 * ("decoder.up_blocks.2.resnets.0.conv1.weight", ...), conv weights in torch [Cout,Cin,3,3] layout. */
typedef struct td_vae td_vae;
typedef struct TdVaeConfig {
  int latent_channels;        /* 16 */
  int out_channels;           /* 3 */
  int num_blocks;             /* 4 */
  int block_out_channels[4];  /* 128,256,512,512 */
  int layers_per_block;       /* 2 */
  int norm_groups;            /* 32 */
} TdVaeConfig;
int td_vae_create(const TdVaeConfig* cfg, int max_latent_h, int max_latent_w, td_vae** out);
void td_vae_destroy(td_vae* f);
int td_vae_num_params(const td_vae* f);
int td_vae_param_info(const td_vae* f, int idx, char* name_buf, int buf_len, int64_t* count);
int td_vae_load_param(td_vae* f, const char* name, const void* src, int64_t count, void* stream);
/* seeded synthetic decoder; std <= 0: 1 / sqrt(fan_in) weights (images with contrast), else that std for every weight and bias */
int td_vae_init_random(td_vae* f, uint64_t seed, float std, void* stream);
/* packed latents bf16 [(h/2)(w/2), 4*latent_channels] (h, w = latent size, both even, within the capacity) -> image_u8 [8h,8w,3]
 * uint8 and/or image_chw bf16 [3,8h,8w] (= vae.decode output); either may be NULL.  The mid-block attention pads its key axis to the next
 * multiple of 64 with exact zeros, so any even h, w is served; with h*w % 64 == 0 there is no pad. */
int td_vae_decode(td_vae* f, const void* packed_latents, int h, int w, float scaling_factor, float shift_factor,
                  void* image_u8, void* image_chw, void* stream);
/* The image size td_vae_decode writes for an h x w latent (2x per block but the last: 8h x 8w for the FLUX.1 VAE) and the channel count of
 * a packed latent row (4 x latent_channels); out pointers may be NULL.  (The torch.ops layer sizes and checks its tensors with it.) */
int td_vae_output_shape(const td_vae* f, int h, int w, int* H, int* W, int* packed_channels);
/* ---- FLUX VAE encoder (AutoencoderKL.encode) and the image-to-image boundaries -----------------------------------------
 * A handle of its own (td_vae_enc), configured by the same TdVaeConfig as the decoder (out_channels = the image's 3 channels,
 * latent_channels = 16 -> 32 moment channels: double_z, no quant_conv).  Parameters use the diffusers names
 * ("encoder.down_blocks.1.downsamplers.0.conv.weight", ...), conv weights in torch [Cout,Cin,3,3] layout. */
typedef struct td_vae_enc td_vae_enc;
#define TD_IMAGE_U8_HWC 0   /* uint8 [H, W, 3] (what PIL gives) */
#define TD_IMAGE_F32_CHW 1  /* float32 [3, H, W] in [0, 1] */
/* Encoder for images of up to max_image_h x max_image_w pixels; every workspace is allocated here ([ext] diffusers 0.31.0
 * vae.py Encoder: conv_in, DownEncoderBlock2D x num_blocks, UNetMidBlock2D with attention, GroupNorm + SiLU, conv_out). */
int td_vae_enc_create(const TdVaeConfig* cfg, int max_image_h, int max_image_w, td_vae_enc** out);
void td_vae_enc_destroy(td_vae_enc* f);
int td_vae_enc_num_params(const td_vae_enc* f);
int td_vae_enc_param_info(const td_vae_enc* f, int idx, char* name_buf, int buf_len, int64_t* count);
int td_vae_enc_load_param(td_vae_enc* f, const char* name, const void* src, int64_t count, void* stream);
/* seeded synthetic encoder, the weight scheme of td_vae_init_random */
int td_vae_enc_init_random(td_vae_enc* f, uint64_t seed, float std, void* stream);
/* `VaeImageProcessor.preprocess(image).to(bf16)` + `vae.encode(x)` up to the posterior's parameters ([ext] autoencoder_kl.py
 * AutoencoderKL._encode): image (device; format TD_IMAGE_*) -> moments_nhwc bf16 [(H/8)(W/8), 2 x latent_channels] = mean | logvar
 * per latent pixel (H/2^(num_blocks-1) for other depths).  H, W multiples of 16 within the capacity; refused before any launch
 * otherwise.  (The mid-block attention pads its key axis to the next multiple of 64 with exact zeros: any such size is served, and a mid-block
 * pixel count that is a multiple of 64 runs unpadded.)  No allocation. */
int td_vae_encode(td_vae_enc* f, const void* image, int image_format, int H, int W, void* moments_nhwc, void* stream);
/* td_vae_encode of `masked_image = image * (1 - mask)` ([ext] diffusers >= 0.32 FluxFillPipeline.__call__; the product is taken in fp32
 * on the preprocessed image and rounded to bf16 by prepare_mask_latents' `.to(dtype)`): the image-in kernel writes bf16(2x - 1) where the
 * binarized mask is 0 and a zero where it is 1 (the zero keeps the sign of 2x - 1, as the fp32 product does).  mask: [H, W] at full pixel
 * resolution, format TD_INPAINT_MASK_* and td_flux_inpaint_mask's binarization (uint8 >= 128, float32 >= 0.5).  Then the encoder as it is. */
int td_vae_encode_masked(td_vae_enc* f, const void* image, int image_format, const void* mask, int mask_format, int H, int W,
                         void* moments_nhwc, void* stream);
/* The moments td_vae_encode writes for an H x W image: h x w latent pixels (H / 2^(num_blocks-1): H/8 for the FLUX.1 VAE) of
 * 2 x latent_channels; out pointers may be NULL.  (The torch.ops layer sizes its output with it.) */
int td_vae_enc_output_shape(const td_vae_enc* f, int H, int W, int* h, int* w, int* moment_channels);
/* moments [h*w, 2C] bf16 (td_vae_encode's output) -> packed FLUX latents [(h/2)(w/2), 4C] bf16, fusing, with the bf16 rounding
 * points of the torch statements: DiagonalGaussianDistribution.sample(eps) (eps NULL: .mode()), FluxImg2ImgPipeline._encode_vae_image
 * ((z - shift_factor) * scaling_factor), FlowMatchEulerDiscreteScheduler.scale_noise (sigma rounded to bf16; noise NULL: no noising)
 * and _pack_latents.  eps / noise: bf16 NCHW [C, h, w] drawn by the caller.  h, w even. */
int td_vae_latents_from_moments(const void* moments, const void* eps, const void* noise, float sigma, float scaling_factor,
                                float shift_factor, int C, int h, int w, void* packed_out, void* stream);
/* VaeImageProcessor.preprocess + .to(bf16) alone: out bf16 [H*W, Cpad] NHWC = RNE(2 x - 1) with x = float32(u8) / 255 or the
 * float32 [0,1] value; channels 3 .. Cpad-1 zero.  Cpad % 8 == 0. */
int td_vae_image_to_nhwc_bf16(const void* image, int image_format, int H, int W, void* out, int Cpad, void* stream);
/* ... of image * (1 - binarize(mask)): the first stage of td_vae_encode_masked alone. */
int td_vae_image_to_nhwc_masked_bf16(const void* image, int image_format, const void* mask, int mask_format, int H, int W, void* out, int Cpad,
                                     void* stream);
/* Downsample2D(use_conv=True, padding=0): F.pad(x, (0,1,0,1)) then a 3x3 conv, stride 2, no padding, as an implicit GEMM:
 *   y[(Hin/2)(Win/2), Cout] = conv3x3_s2(x[Hin*Win, Cin]) + bias;   Hin, Win even, Cin % 64 == 0, w packed as for td_conv3x3_nhwc_bf16. */
int td_conv3x3_s2_nhwc_bf16(const void* x, const void* w, const void* bias, void* y, int Hin, int Win, int Cin, int Cout, void* stream);
/* GroupNorm (+ optional SiLU) over an NHWC image x[P,C]; workspace: td_groupnorm_workspace_floats() floats. */
int td_groupnorm_nhwc_bf16(const void* x, void* y, int P, int C, int groups, float eps, const void* gamma,
                           const void* beta, int silu, float* workspace, void* stream);
int td_groupnorm_workspace_floats(void);
/* p[rows,cols] (bf16) = softmax(scale * s[rows,cols]) (fp32 in). */
/* (s 16-byte, p 8-byte aligned, neither NULL: the kernel's vector accesses need it; refused with TD_ERR_INVALID otherwise)
 * scale must be finite and > 0 (td_abi_version() >= 17: TD_ERR_INVALID otherwise): the row maximum is taken over the unscaled scores, which is the
 * maximum of scale * s only for a positive scale. */
int td_softmax_rows_f32_bf16(const float* s, void* p, int rows, int cols, float scale, void* stream);
/* ... with rows `ld` elements apart in both matrices (ld >= cols, ld % 4 == 0): softmax over the first `cols` columns of each row, the pad
 * columns [cols, ld) of s never read and those of p written as exact zeros (the VAE mid-block attention's key-axis pad). */
int td_softmax_rows_strided_f32_bf16(const float* s, void* p, int rows, int cols, int ld, float scale, void* stream);

/* ---- Qwen2-VL text decoder: hidden states at `model.norm` + KV-cached decoding -------------------------
 * Replaces the vLLM fork's model runner behind `self.mllama.generate(inputs, sampling_params)` with
 * `return_hidden_states=True` (thinkdiff/models/mllama_vllm_t5_embed_decoder_2.py:790-816,1083-1089;
 * thinkdiff/models/mllama_vllm_generate_1.py:382-413,586,614-615): `prompt_hidden_states` /
 * `outputs[0].hidden_states` are `hidden_out` of the prompt tokens / of the generated tokens.
 * Parameters use the Hugging Face names (model.embed_tokens.weight, model.layers.N.self_attn.q_proj.weight,
 * ..., model.norm.weight, lm_head.weight). */
typedef struct td_qwen2 td_qwen2;
typedef struct TdQwen2Config {
  int hidden;            /* 3584 (7B) / 1536 (2B) */
  int num_layers;        /* 28 */
  int num_heads;         /* 28 / 12 */
  int num_kv_heads;      /* 4 / 2 */
  int head_dim;          /* 128 */
  int intermediate;      /* 18944 / 8960 */
  int vocab;             /* 152064 / 151936 */
  int tie_embeddings;    /* 0 / 1 */
  int mrope_section[3];  /* 16,24,24 */
  float rms_eps;         /* 1e-6 */
  float rope_theta;      /* 1e6 */
} TdQwen2Config;

int td_qwen2_create(const TdQwen2Config* cfg, int max_tokens, td_qwen2** out);
void td_qwen2_destroy(td_qwen2* f);
int td_qwen2_num_params(const td_qwen2* f);
int td_qwen2_param_info(const td_qwen2* f, int idx, char* name_buf, int buf_len, int64_t* count);
int td_qwen2_load_param(td_qwen2* f, const char* name, const void* src, int64_t count, void* stream);
int td_qwen2_init_random(td_qwen2* f, uint64_t seed, float std, void* stream);
/* n new tokens at cache positions [pos0, pos0+n): token_ids int32[n] OR inputs_embeds bf16[n,hidden] (device),
 * position_ids int32[3,n] (M-RoPE t/h/w streams, device); hidden_out bf16[n,hidden] = model.norm output (may be
 * NULL); logits_last bf16[vocab] of the last token (may be NULL).  pos0 = 0 is a prefill; pos0 > 0 continues. */
int td_qwen2_forward(td_qwen2* f, const int* token_ids, const void* inputs_embeds, const int* position_ids, int n,
                     int pos0, void* hidden_out, void* logits_last, void* stream);
/* td_qwen2_forward on sequence `slot` of a handle partitioned by td_qwen2_set_slots (td_qwen2_forward = slot 0). */
int td_qwen2_forward_slot(td_qwen2* f, int slot, const int* token_ids, const void* inputs_embeds, const int* position_ids, int n,
                          int pos0, void* hidden_out, void* logits_last, void* stream);
/* Batched KV-cached decode (the precompute job, mllama_vllm_generate_1.py:585: vLLM decodes its whole request batch together):
 * the cache of max_tokens rows per layer is split into n_slots sequences of max_tokens / n_slots rows. */
int td_qwen2_create_slots(const TdQwen2Config* cfg, int slot_len, int n_slots, td_qwen2** out);   /* n_slots sequences of slot_len tokens */
/* ... and an activation workspace of ws_rows rows (>= slot_len): the capacity of a batched prefill, B x L <= ws_rows */
int td_qwen2_create_ex(const TdQwen2Config* cfg, int slot_len, int n_slots, int ws_rows, td_qwen2** out);
/* Prefill B right-padded sequences (row b*L + t) into slots 0..B-1 in one pass; lens[b] = real tokens (HOST ints);
 * hidden_out bf16[B*L,hidden], logits_last bf16[B,vocab] of each sequence's last real token (either may be NULL). */
int td_qwen2_prefill_batch(td_qwen2* f, int B, int L, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                           const int* lens, void* hidden_out, void* logits_last, void* stream);
/* ... into slots slot0..slot0+B-1: a request batch with B x L above ws_rows is prefilled in several calls */
int td_qwen2_prefill_batch_at(td_qwen2* f, int slot0, int B, int L, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                              const int* lens, void* hidden_out, void* logits_last, void* stream);
/* Packed prefill: the B prompts lie back to back -- rows [sum(lens[:b]), sum(lens[:b+1])) belong to sequence b, no padding rows -- and go to cache
 * slots slot0 .. slot0 + B - 1: what vLLM's scheduler does with the reference's request batches (max_num_batched_tokens rows per pass,
 * configs/qwen2_vl_embed_ccsbu.yaml:19; thinkdiff/models/mllama_vllm_generate_1.py:585).  total = sum(lens) <= the handle's workspace rows.
 * token_ids int32[total] or inputs_embeds bf16[total, hidden]; position_ids int32[3, total]; lens HOST int[B]; hidden_out bf16[total, hidden];
 * logits_last bf16[B, vocab] of each prompt's last token (either output may be NULL). */
int td_qwen2_prefill_packed(td_qwen2* f, int slot0, int B, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                            const int* lens, void* hidden_out, void* logits_last, void* stream);
/* ... sequence b into cache slot slots[b] (HOST ints, distinct, any order): the free slots of a running batch (continuous batching). */
int td_qwen2_prefill_packed_slots(td_qwen2* f, int B, const int* slots, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                                  const int* lens, void* hidden_out, void* logits_last, void* stream);
/* ... behind cached prefixes (td_abi_version() >= 23; vLLM's automatic prefix caching needs it): sequence b feeds lens[b] >= 1 NEW rows, which go to cache
 * rows [prefix_lens[b], prefix_lens[b] + lens[b]) of slot slots[b].  The caller vouches that the first prefix_lens[b] rows of that slot hold the keys and
 * values of the tokens in front (same tokens, same position ids: the cached keys are rotated).  token_ids / inputs_embeds / position_ids / hidden_out /
 * logits_last cover the new rows only, laid out as in td_qwen2_prefill_packed_slots; lens and prefix_lens are HOST ints.  Every prefix_lens[b] == 0: that
 * entry itself, launch for launch.  bf16 cache: the attention reads K / V straight from the cache (td_attention_prefix_segments_bf16's form).  e4m3 cache:
 * staged -- rows [0, prefix + len) of every sequence are dequantised into a buffer of ws_rows rows (allocated at the first such call), so a pass with
 * sum(prefix_lens + lens) > ws_rows is refused.  TD_ERR_INVALID naming the value: a null argument, B outside 1 .. 256, a slot out of range or given twice,
 * lens[b] < 1, prefix_lens[b] < 0, prefix_lens[b] + lens[b] above the slot capacity, sum(lens) > ws_rows. */
int td_qwen2_prefill_packed_prefix_slots(td_qwen2* f, int B, const int* slots, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                                         const int* lens, const int* prefix_lens, void* hidden_out, void* logits_last, void* stream);
int td_qwen2_set_slots(td_qwen2* f, int n_slots);   /* re-partition the cache rows of an existing handle */
/* Decode step: the rotary embedding of the new q / k rows and the write of the new k | v rows into the cache happen inside the decode-attention
 * launch (default, one launch per layer fewer) or in a launch of their own (on = 0: A/B and the bit-identity test).  Same arithmetic either way
 * (the vLLM fork's rotary_emb + cache write, thinkdiff/models/mllama_vllm_t5_embed_decoder_2.py:1083).  Returns the previous setting. */
int td_qwen2_set_fused_rope(td_qwen2* f, int on);
int td_qwen2_slot_capacity(const td_qwen2* f);
/* copy the first `len` cache rows of sequence src to sequence dst (compaction when a sequence finishes) */
int td_qwen2_move_slot(td_qwen2* f, int src, int dst, int len, void* stream);
/* KV fork (td_abi_version() >= 16; csrc/kv_fork.hip): the first n_rows rows of slot src_slot copied to the same rows of every dst_slots[i], for all
 * planes in ONE launch; every source chunk is loaded once and stored n_dst times.  A plane is a device array of slots x slot_rows rows of row_bytes
 * bytes: slot s starts at base + s * slot_rows * row_bytes.  Accesses are 16 bytes wide wherever the slot stride is a multiple of 16 (8, 4 or 2
 * bytes otherwise: the width every slot's start shares), with 2-byte pieces in front of the first and behind the last aligned address.
 * planes and dst_slots are HOST arrays, read before the call returns: they reach the device in the launches' own arguments (64 planes x 192
 * destinations per launch), so the call allocates nothing, synchronises nothing and no host buffer has to outlive it.  The caller vouches that
 * every named slot lies inside its plane.  TD_ERR_INVALID with a message naming the value, before any HIP call: a NULL planes / dst_slots / base,
 * n_planes < 1, n_dst < 1, n_rows < 0 or above a plane's slot_rows, a negative slot, src_slot among the destinations, a destination given twice,
 * row_bytes not a positive multiple of 2, a base that is not 2-byte aligned.  n_rows == 0: TD_OK, no launch. */
typedef struct {
  void* base;
  int64_t row_bytes;
  int64_t slot_rows;
} TdKvPlane;
int td_kv_fork_rows(const TdKvPlane* planes, int n_planes, int src_slot, const int* dst_slots, int n_dst, int n_rows, void* stream);
/* td_kv_fork_rows over the handle's own planes (one bf16 plane per layer; the byte plane and the scale plane per layer on the e4m3 cache): the first
 * `len` cache rows of sequence src to every sequence dst_slots[0 .. n_dst) (HOST ints) -- n sequences continuing from one prefill.  Also refused:
 * a slot outside [0, n_slots), len above the slot capacity.  td_qwen2_move_slot is the one-destination form on hipMemcpyAsync. */
int td_qwen2_fork_slot(td_qwen2* f, int src, const int* dst_slots, int n_dst, int len, void* stream);
/* KV gather (td_abi_version() >= 18; csrc/kv_fork.hip): for every row j of 0 .. n with copy_src_dev[j] >= 0, the first n_rows[j] rows of slot
 * slots[copy_src_dev[j]] copied to the same rows of slot slots[j], on every plane -- the reordering of cache slots behind a beam-search step, whose
 * sources only the device knows.  slots and n_rows are HOST int arrays of n entries, read before the call returns (they travel in the launches' own
 * arguments: 64 planes x 64 destination rows per launch, every launch with the whole slot table); copy_src_dev is a DEVICE int32[n] read by the
 * kernel: -1 (any negative value), j itself or a value >= n copies nothing, and a workgroup of such a row returns at once.  Access widths and the
 * head / body / tail split are td_kv_fork_rows'.  CONTRACT: the caller vouches that no destination slot (a row with copy_src >= 0) is the source of
 * another row of the same call -- td_beam_select's placement guarantees it -- and that every slot lies inside its plane.  TD_ERR_INVALID with a
 * message naming the value, before any HIP call: a NULL planes / slots / copy_src_dev / n_rows / base, n_planes < 1, n outside 1..256, a negative
 * slot, a slot given twice, n_rows negative or above a plane's slot_rows, row_bytes not a positive multiple of 2, a base that is not 2-byte aligned.
 * Every n_rows == 0: TD_OK, no launch. */
int td_kv_gather_rows(const TdKvPlane* planes, int n_planes, int n, const int* slots, const int32_t* copy_src_dev, const int* n_rows, void* stream);
/* td_kv_gather_rows over the handle's own planes (bf16, or bytes and scales of the e4m3 cache): sequence slots[j] takes the first lens[j] cache rows
 * of sequence slots[copy_src_dev[j]].  Also refused: a slot outside [0, n_slots), a len above the slot capacity. */
int td_qwen2_gather_slots(td_qwen2* f, int n, const int* slots, const int32_t* copy_src_dev, const int* lens, void* stream);
/* One new token for each of the sequences in slots 0..B-1 (B <= 64) in one pass over the weights: token_ids int32[B],
 * position_ids int32[3,B] (device); cache_pos[b] = tokens already cached for sequence b (HOST ints); hidden_out bf16[B,hidden],
 * logits bf16[B,vocab] (either may be NULL). */
int td_qwen2_decode_batch(td_qwen2* f, int B, const int* token_ids, const int* position_ids, const int* cache_pos,
                          void* hidden_out, void* logits, void* stream);
/* td_qwen2_decode_batch for the sequences in cache slots slots[0 .. B-1] (HOST ints, distinct; NULL = 0 .. B-1); row b of token_ids / position_ids /
 * cache_pos / hidden_out / logits belongs to slot slots[b].  A finished sequence then frees its slot without any cache rows being moved and a waiting
 * request is prefilled into it (td_qwen2_prefill_packed_slots): vLLM's continuous batching of the reference's request batches
 * (thinkdiff/models/mllama_vllm_generate_1.py:585, `max_num_seqs: 256`), with whole-sequence slots in place of paged blocks. */
int td_qwen2_decode_batch_slots(td_qwen2* f, int B, const int* slots, const int* token_ids, const int* position_ids, const int* cache_pos,
                                void* hidden_out, void* logits, void* stream);
/* out bf16[n,hidden] = embed_tokens[token_ids] (device int32[n]): the host splices vision tokens into this to form inputs_embeds. */
int td_qwen2_embed_tokens(td_qwen2* f, const int* token_ids, void* out, int n, void* stream);

/* ---- 8-bit weight stream (td_abi_version() >= 12): weight-only quantisation of the decoder's Linears -----------------------------------------
 * Format (fixed): OCP e4m3 bytes with ONE POWER-OF-TWO scale per output row of a Linear weight W[N, K]:
 *   amax_n = max_k |W[n, k]|;  e_n = the smallest integer with amax_n 2^-e_n <= 448, clamped to [-40, 40] (0 for an all-zero row);
 *   q[n, k] = e4m3_rne(W[n, k] 2^-e_n) (the product is exact in fp32: one rounding);  W^[n, k] = q[n, k] 2^e_n.
 * W^ is a bf16 value exactly (4 significant bits, exponent inside bf16's range), so the quantised model is an ordinary bf16 model with weights W^,
 * and the stream kernels reproduce those bf16 values from the bytes inside the conversion instruction: the products of a dot product are the
 * ones the bf16 kernels form on W^, only the order of the fp32 sum may differ.  Activations, KV cache, norms and attention stay bf16. */
/* w bf16 [N, ldw] -> q bytes [N, K] (row stride K), scale fp32 [N] = 2^e_n, and w_hat bf16 [N, ldw] = W^ (NULL: not written; may alias w).
 * K % 8 == 0, ldw % 8 == 0, ldw >= K; w / w_hat 16-byte, q 8-byte, scale 4-byte aligned.  TD_ERR_INVALID before any HIP call otherwise.
 * A row whose exponent is clamped at +40 (amax > 448 x 2^40) saturates at +-448 x 2^40. */
int td_quant_weight_rows_e4m3(const void* w, int64_t ldw, void* q, float* scale, void* w_hat, int N, int K, void* stream);
/* y[M, N] = epilogue(x[M, K] . W^[N, K]^T) with W^ given as (wq, w_scale) in the format above: td_linear_bf16's epilogue and rounding points (bias,
 * act, gate, res).  M <= 64 ONLY (the weight-stream kernels; more rows read W^ as bf16 through td_linear_bf16).  N % 4 == 0 and K % 16 == 0; more than
 * 16 rows (and 5 .. 16 rows on the matrix core) need K % 128 == 0, N % 16 == 0, ldy % 4 == 0.  x and wq 16-byte aligned, ldx % 8 == 0.  M > 64, a NULL
 * x / wq / w_scale / y, misaligned operands or a K the kernels do not take: TD_ERR_INVALID with a message, before any HIP call. */
int td_linear_w8_bf16(const void* x, int64_t ldx, const void* wq, const float* w_scale, const void* bias, void* y, int64_t ldy,
                      int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr, void* stream);
/* ... with td_linear_split_bf16's two outputs (columns < n_split -> y0 with act0, the rest -> y1 with act1; n_split % 4 == 0) */
int td_linear_split_w8_bf16(const void* x, int64_t ldx, const void* wq, const float* w_scale, const void* bias, void* y0, int64_t ldy0, int act0,
                            void* y1, int64_t ldy1, int act1, int M, int N, int K, int n_split, void* stream);
/* Gated MLP front in one pass, the decode step's form: w = [gate rows | up rows] ([2 I, K]), y[m, n] = bf16(bf16(silu(bf16(x . gate_n))) * bf16(x . up_n)),
 * n < I -- Linear, SiLU and product each round, as td_linear_bf16 + td_silu_mul_bf16 do.  M <= 64, I % 8 == 0, ldy % 4 == 0; bf16: K % 8 == 0
 * (more than 16 rows: K % 64 == 0); w8: K % 16 == 0 (more than 16 rows: K % 128 == 0).  TD_ERR_INVALID before any HIP call otherwise. */
int td_linear_glu_bf16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int M, int I, int K, void* stream);
int td_linear_glu_w8_bf16(const void* x, int64_t ldx, const void* wq, const float* w_scale, void* y, int64_t ldy, int M, int I, int K, void* stream);

/* ---- 4-bit weight stream (td_abi_version() >= 20; vLLM's `quantization="mxfp4"`): the same weight-only scheme one format down ------------------------
 * Format (fixed): OCP MXFP4 -- e2m1 elements under ONE e8m0 POWER-OF-TWO scale per block of 32 consecutive k of an output row of W[N, K], K % 32 == 0:
 *   amax = max |w| over the block;  e = floor(log2(amax)) - 2 (OCP MX v1.0), clamped to [-64, 64] (0 for an all-zero block);
 *   q = e2m1_rne(w 2^-e): round to nearest, ties to the even code, saturated at +-6 (scaled values in (6, 8) clip to 6); the grid is
 *   {0, 0.5, 1, 1.5, 2, 3, 4, 6} with a sign bit, and -0 keeps it;  W^ = q 2^e.
 * Storage: packed uint8 [N, K / 2], element 2j in the LOW nibble of byte j (OCP, torch's float4_e2m1fn_x2, what Quark / torchao write); scales uint8
 * [N, K / 32] = e + 127.  W^ is a bf16 value exactly (2 significant bits), so again the quantised model is an ordinary bf16 model with weights W^, and the
 * stream kernels rebuild those bf16 values inside the conversion instruction: only the order of the fp32 sum may differ from the bf16 kernels on W^. */
/* w bf16 [N, ldw] -> packed [N, K / 2], scales [N, K / 32] (both dense), and w_hat bf16 [N, ldw] = W^ (NULL: not written; may alias w).
 * K % 32 == 0, ldw % 8 == 0, ldw >= K; w / w_hat / packed 16-byte aligned.  TD_ERR_INVALID before any HIP call otherwise. */
int td_quant_weight_rows_mxfp4(const void* w, int64_t ldw, void* packed, void* scales, void* w_hat, int N, int K, void* stream);
/* packed, scales -> w_hat bf16 [N, ldw] = W^, exactly (any scale byte in [1, 254] whose W^ stays inside bf16: a checkpoint written under another scale
 * rule dequantises to its own values).  The same argument rules. */
int td_dequant_rows_mxfp4(const void* packed, const void* scales, void* w_hat, int64_t ldw, int N, int K, void* stream);
/* td_linear_w8_bf16 / td_linear_split_w8_bf16 / td_linear_glu_w8_bf16 with W^ given as (packed, scales) in the format above: the same arguments, epilogues
 * and rounding points.  M <= 64 ONLY.  N % 4 == 0 and K % 32 == 0; more than 16 rows (and 3 .. 16 rows on the matrix core) need K % 256 == 0 (a 128-byte
 * line of a packed row), N % 16 == 0, ldy % 4 == 0.  x and packed 16-byte aligned, scales 8-byte, ldx % 8 == 0.  M > 64, a NULL x / packed / scales / y,
 * misaligned operands or a K the kernels do not take: TD_ERR_INVALID with a message, before any HIP call. */
int td_linear_w4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* bias, void* y, int64_t ldy,
                      int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr, void* stream);
int td_linear_split_w4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* bias, void* y0, int64_t ldy0, int act0,
                            void* y1, int64_t ldy1, int act1, int M, int N, int K, int n_split, void* stream);
int td_linear_glu_w4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, void* y, int64_t ldy, int M, int I, int K, void* stream);

/* ---- grouped int4 weight stream (td_abi_version() >= 22): AWQ / GPTQ checkpoints, loaded as they are --------------------------------------------------
 * Format (fixed): asymmetric uint4 under ONE fp16 scale and ONE 4-bit zero point per group of G consecutive k of an output row of W[N, K]; G is 32, 64 or
 * 128, K % G == 0 and K % 32 == 0:   q, z in 0 .. 15, s a finite fp16;   W^ = bf16_rne(fp32(q - z) * fp32(s)).
 * q - z has at most 5 significant bits and s has 11: the product is exact in fp32, the rounding to bf16 is the ONLY rounding, and |W^| <= 15 * 65504 is
 * finite in bf16 (an fp16 subnormal scale gives a normal bf16 magnitude).  So once more the quantised model is an ordinary bf16 model with weights W^:
 * td_dequant_rows_int4 and the stream kernels apply the same rounding and agree bit for bit WITH EACH OTHER; against the formula they differ in one
 * case that no value can show: a zero weight (q == z) under a negative scale is +0 here where the formula's product is -0.
 * Storage: packed uint8 [N, K / 2], scales fp16 [N, K / G], zeros uint8 [N, K / G] (values 0 .. 15; only the low nibble is read), all dense.  The order of
 * the nibbles inside `packed` belongs to the library (csrc/int4_group.h): packed bytes are made by td_repack_int4 and by nothing else. */
enum { TD_INT4_AWQ = 0, TD_INT4_GPTQ = 1, TD_INT4_GPTQ_V2 = 2 /* flag, with TD_INT4_GPTQ: checkpoint_format "gptq_v2", zero points stored as they are */ };
/* One checkpoint Linear -> the device layout, in one launch (all pointers device memory).
 *   TD_INT4_AWQ, AutoAWQ version "GEMM": qweight int32 [K, N / 8], nibble p of column c = q[k, 8c + o[p]], o = {0, 2, 4, 6, 1, 3, 5, 7}; qzeros int32
 *     [K / G, N / 8] packed the same way; scales_in fp16 [K / G, N].  The Linear is x @ w with w[k, n] = (q - z) s, so row n of W is w[:, n].
 *   TD_INT4_GPTQ, AutoGPTQ 4-bit: qweight int32 [K / 8, N], nibble p of row r = q[8r + p, n]; qzeros int32 [K / G, N / 8], nibble p of column c =
 *     z[g, 8c + p] - 1 (z = (stored + 1) & 15, AutoGPTQ's own unpack) -- with TD_INT4_GPTQ | TD_INT4_GPTQ_V2: z = stored; scales_in fp16 [K / G, N].
 * g_idx (int32 [K], may be NULL) is NOT read: only the trivial map g_idx[k] = k / G is served (no act-order), and the caller vouches for it.
 * N % 8 == 0; qweight / qzeros / packed 4-byte aligned.  TD_ERR_INVALID with a message, before any HIP call, otherwise. */
int td_repack_int4(int layout, const void* qweight, const void* qzeros, const void* scales_in, const void* g_idx, int N, int K, int G,
                   void* packed, void* scales, void* zeros, void* stream);
/* packed, scales, zeros -> w_hat bf16 [N, ldw] = W^.  ldw % 8 == 0, ldw >= K; w_hat 16-byte aligned, packed 4-byte. */
int td_dequant_rows_int4(const void* packed, const void* scales, const void* zeros, int G, void* w_hat, int64_t ldw, int N, int K, void* stream);
/* td_linear_w4_bf16 / td_linear_split_w4_bf16 / td_linear_glu_w4_bf16 with W^ given as (packed, scales, zeros, G) in the format above: the same arguments,
 * epilogues, rounding points and refusals.  M <= 64 ONLY.  N % 4 == 0, K % G == 0 and K % 32 == 0; more than 16 rows (and 3 .. 16 rows on the matrix core)
 * need K % 256 == 0, N % 16 == 0, ldy % 4 == 0.  x, packed and scales 16-byte aligned, zeros 8-byte, ldx % 8 == 0. */
int td_linear_i4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* zeros, int G, const void* bias, void* y, int64_t ldy,
                      int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr, void* stream);
int td_linear_split_i4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* zeros, int G, const void* bias, void* y0,
                            int64_t ldy0, int act0, void* y1, int64_t ldy1, int act1, int M, int N, int K, int n_split, void* stream);
int td_linear_glu_i4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* zeros, int G, void* y, int64_t ldy, int M, int I,
                          int K, void* stream);

enum { TD_QWEN2_WEIGHTS_BF16 = 0, TD_QWEN2_WEIGHTS_E4M3 = 1, TD_QWEN2_WEIGHTS_MXFP4 = 2, TD_QWEN2_WEIGHTS_INT4 = 3 };
/* TD_QWEN2_WEIGHTS_INT4 is not a mode td_qwen2_quantize_weights takes (there is no round-to-nearest int4 quantiser): a handle enters it by being LOADED
 * with int4 Linears.  `name` is a decoder Linear's "...weight" name from td_qwen2_param_info (q / k / v / o / gate / up / down_proj); packed / scales / zeros
 * are that Linear's device layout from td_repack_int4 (device memory).  The call writes W^ into the rows of the bf16 arena td_qwen2_load_param would write
 * for that name, and the nibbles, scales and zeros into the same rows of the handle's int4 copy (allocated on the first call from the shapes of all
 * 7 x layers Linears: N K / 2 + 3 N K / G bytes each, 0.26x the bf16 Linear weights at G = 128, beside the arena).  Until every one of the 7 x layers
 * Linears has int4 data the handle is stale: every run is refused.  Then the mode is TD_QWEN2_WEIGHTS_INT4 and the weight stream is on, with
 * td_qwen2_set_weight_stream, td_qwen2_weight_info (n_linears = 7 x layers) and td_qwen2_weight_stream_launches as in the other modes.  With the stream
 * on, only the row counts at which the int4 forms measured faster than the bf16 kernels read the copy (the table int4_rows_routed in
 * csrc/qwen2_engine.hip, from profiles/qwen2_int4_bench.json; td_qwen2_set_int4_routing below lifts it); every other launch reads W^ from the bf16
 * arena -- the same model.  lm_head and the
 * embedding table are not quantised in these checkpoints: they load through td_qwen2_load_param and always run as bf16.
 * Mixing is refused with TD_ERR_INVALID, the message naming the rule: this call on an E4M3 / MXFP4 handle; a second G on one handle;
 * td_qwen2_quantize_weights, td_qwen2_init_random, or td_qwen2_load_param of a decoder Linear weight on an INT4 handle (biases, norms, embeddings and
 * lm_head load as ever). */
int td_qwen2_load_param_int4(td_qwen2* f, const char* name, const void* packed, const void* scales, const void* zeros, int G, void* stream);
/* Measurement and test switch on an INT4 handle (as td_attention_verify_set_form is for the verify kernels): all = 1 sends EVERY launch of up to 64 rows
 * that the int4 forms take to the int4 copy while the stream is on, all = 0 (the default) only the row counts of the table above.  The model is the same
 * either way.  tools/bench_qwen2_int4.py times both settings, which is where the table comes from.  Drops the captured decode graphs.  Returns the
 * previous setting (0 / 1); TD_ERR_INVALID for another value, a NULL handle or a handle that is not in INT4 mode. */
int td_qwen2_set_int4_routing(td_qwen2* f, int all);
/* Called after the parameters are loaded.  mode = TD_QWEN2_WEIGHTS_E4M3 or TD_QWEN2_WEIGHTS_MXFP4 (anything else: TD_ERR_INVALID; below, "8-bit copy" reads
 * "4-bit copy": packed nibbles + block scale bytes, 0.27x the Linear weights instead of half).  A handle quantised in one mode REFUSES the other
 * (TD_ERR_INVALID naming both) until its parameters are loaded again: the original weights are gone.  Builds the 8-bit copy and the row scales of every
 * layer's q|k|v, o, gate|up and down weights and of lm_head (4 x layers + 1 Linears) and OVERWRITES the bf16 weights with W^; with tied embeddings the
 * embedding table IS the lm_head weight and becomes W^ too.  From then on the weight stream is on: every Linear launch of up to 64 rows that the
 * weight-stream kernels take (the decode step of 1 .. 64 sequences, lm_head, prefills of up to 64 rows) reads the 8-bit copy; launches of more rows
 * (prefill, packed prefill, the 65 .. 256-sequence decode step) read W^ as bf16 and do not depend on the switch at all.  Memory GROWS by half the
 * Linear weights (the copy sits beside the bf16 arena: this buys time, not memory).  Drops the captured decode graphs.  May be called again
 * (idempotent: quantising W^ gives W^) and MUST be called again after td_qwen2_load_param / td_qwen2_init_random on a quantised handle: until then
 * every forward, prefill and decode entry, and td_qwen2_embed_tokens (with tied embeddings its table is a quantised weight; it refuses on an
 * untied model too, one rule for the handle), returns TD_ERR_INVALID naming this function -- never a run on a half-quantised model.
 * Allocates on the first call (not capturable). */
int td_qwen2_quantize_weights(td_qwen2* f, int mode, void* stream);
/* A/B switch and test handle on a quantised handle: on (default after quantising) = launches of up to 64 rows read the 8-bit copy, off = the same
 * launches read bf16 W^.  The model is the same either way.  Two exceptions to "the same launches", both in the decode step: with hidden >= 3072 a
 * step of 33 .. 64 sequences runs on the weight-stream kernels with the stream on and on the tile / split-K kernels with it off (the bf16
 * cross-over of that width is 32 sequences; on half the bytes the stream stays ahead through 64), and with hidden < 3072 a step of exactly 2
 * sequences reads bf16 W^ even with the stream on (measured slower on the bytes, on the 2B shape only).  Drops the captured decode graphs.
 * Returns the previous setting (0 / 1); TD_ERR_INVALID on a NULL or unquantised handle. */
int td_qwen2_set_weight_stream(td_qwen2* f, int on);
/* mode (TD_QWEN2_WEIGHTS_*), whether the stream is on, bytes of the 8-bit copy (weight bytes + row scales; MXFP4: N K / 2 + N K / 32 per Linear), number
 * of quantised Linears; any output may be NULL */
int td_qwen2_weight_info(const td_qwen2* f, int* mode, int* stream_on, int64_t* bytes_8bit, int* n_linears);
/* How many Linear launches the handle has enqueued so far that read the 8-bit copy (a captured decode step counts once, when it is captured;
 * its replays launch nothing from the host and do not count).  The test handle that tells "the 8-bit kernels ran" from "the bf16 kernels ran on
 * W^", which the outputs alone cannot (the model is the same).  -1 on a NULL handle. */
int64_t td_qwen2_weight_stream_launches(const td_qwen2* f);

/* ---- per-request LoRA (td_abi_version() >= 24; vLLM's `enable_lora` with a LoRARequest per request) ------------------------------------------------
 * UNMERGED adapters: every row of a prefill or a decode step names its own adapter (or none), and td_lora_rows_bf16 adds that adapter's low-rank update
 * behind each base Linear of a layer (q | k | v in front of RoPE, o_proj, gate | up in front of SiLU * up, down_proj).  The base Linears are the launches
 * they were, so every weight-stream mode and both cache formats work underneath; lm_head and the embeddings are never adapted.  A pass in which no row names
 * an adapter -- and every pass of a handle on which LoRA is not enabled -- issues exactly the launches it issued before and returns the same bits.
 * A decode step with an adapted row takes a launch list of its own (gate | up into the [B, 2 I] buffer, SiLU * up in its own launch, the wide path's RMSNorm
 * out of the split-K reduction), captured under a graph key of its own; the row -> adapter array is device data, so the captured step replays under a
 * changed assignment.  The rows' adapters come from a host map cache slot -> adapter:
 *   td_qwen2_lora_set_slot sets it (index -1: none); td_qwen2_fork_slot and td_qwen2_move_slot give the destination the source's adapter;
 *   td_qwen2_set_slots clears it; td_qwen2_gather_slots cannot know its sources: the caller sets all beams of a request to the request's adapter first. */
/* Allocates the pool (max_loras <= TD_LORA_MAX_ADAPTERS adapters x layers x 7 Linears, each place sized for max_rank <= TD_LORA_ROWS_MAX_RANK) and the
 * kernels' workspace for the handle's workspace rows.  Once per handle; not capturable; drops the step graphs. */
int td_qwen2_lora_enable(td_qwen2* f, int max_loras, int max_rank);
/* One pair of adapter `index` (0 .. max_loras - 1): `module` is the Hugging Face name of one of the 7 Linears of a layer ("model.layers.3.self_attn.q_proj",
 * ..., "model.layers.3.mlp.down_proj"), A = lora_A.weight [rank, K], B = lora_B.weight [N, rank], device bf16 (the caller vouches for the extents: N, K are
 * the module's), scale = lora_alpha / rank (or / sqrt(rank)).  One rank and scale per adapter.  A module an adapter never loads stays untouched for its rows.
 * Packs into the pool on `stream`; drops the step graphs. */
int td_qwen2_lora_load(td_qwen2* f, int index, const char* module, const void* A, const void* B, int rank, float scale, void* stream);
/* Forgets every pair of adapter `index`; slots that named it name none.  Drops the step graphs. */
int td_qwen2_lora_remove(td_qwen2* f, int index);
int td_qwen2_lora_set_slot(td_qwen2* f, int slot, int index);
/* max_loras (0: not enabled), adapters holding at least one pair, bytes held (pool + workspace), and the low-rank launches enqueued or captured so far
 * (two per adapted Linear: the count td_qwen2_weight_stream_launches keeps for the 8-bit stream; an adapter-less pass adds none); any output may be NULL */
int td_qwen2_lora_info(const td_qwen2* f, int* max_loras, int* resident, int64_t* bytes, int64_t* launches);

/* ---- e4m3 KV cache (td_abi_version() >= 13; vLLM's `kv_cache_dtype="fp8"`) --------------------------------------------------------------------
 * Format (fixed): the weight format above applied to every 128-wide head vector x of a cache row (one token of one sequence, one layer; the rotated
 * k | v row of 2 Hkv head vectors):
 *   amax = max_d |x_d|;  e = the smallest integer with amax 2^-e <= 448, clamped to [-40, 40] (0 for an all-zero vector);
 *   q_d = e4m3_rne(x_d 2^-e) (OCP e4m3, saturating at +-448; the product is exact in fp32: one rounding);  x^_d = q_d 2^e.
 * Per layer a BYTES plane [max_tokens, 2 Hkv 128] u8 (k heads then v heads, the column order of the bf16 row) and a SCALE plane fp32 [max_tokens, 2 Hkv]
 * holding 2^e (column h = k head h, column Hkv + h = v head h): KVW + 8 Hkv bytes per row against 2 KVW (KVW = 2 Hkv 128), a ratio of 0.516.
 * x^ is a bf16 value exactly, so a handle in this mode is an ordinary bf16 engine whose cache holds K^ | V^, and EVERY consumer sees those values:
 * the decode step, the prefill's own attention (the rows are rounded before it runs) and a continued td_qwen2_forward.  A result never depends on whether
 * a key came from registers, the staging rows or the cache.  The scales are powers of two, so the kernels fold them inside the conversion instructions
 * (v_cvt_scalef32_pk_bf16_fp8 for k into v_dot2c, v_cvt_scalef32_pk_f32_fp8 for v): exact, the arithmetic from there on is that of the bf16 kernel.
 * DEVIATION from vLLM: vLLM stores e4m3 under ONE per-tensor scale (1.0 without calibration).  Here every (token, kv head, k or v) has its own scale, 3 %
 * of the bytes, which removes the saturation and underflow risk of an uncalibrated scale on Qwen2's large rotated keys.
 * The tile (prefill) attention does not read this format: prefills attend over bf16 staging rows that hold the same values. */
enum { TD_QWEN2_KV_BF16 = 0, TD_QWEN2_KV_E4M3 = 1 };
/* td_qwen2_create_ex with the cache format; fixed at creation because it sizes the allocation (TD_QWEN2_KV_E4M3: the bf16 cache is not allocated).
 * td_qwen2_create_ex equals kv_mode = TD_QWEN2_KV_BF16.  Any other mode: TD_ERR_INVALID before anything is allocated.  Independent of
 * td_qwen2_quantize_weights.  td_qwen2_init_random draws the same weights for the same seed in both modes. */
int td_qwen2_create_kv(const TdQwen2Config* cfg, int slot_len, int n_slots, int ws_rows, int kv_mode, td_qwen2** out);
/* mode (TD_QWEN2_KV_*), bytes of one cache row of one layer, bytes of the whole handle's cache (rows x layers); any output may be NULL */
int td_qwen2_kv_info(const td_qwen2* f, int* kv_mode, int64_t* bytes_per_row, int64_t* cache_bytes);
/* rows [row0, row0 + n) of sequence `slot` in layer `layer` -> out_bf16 [n, 2 Hkv 128] (device, 16-byte aligned): dequantised (exact); bf16 mode: a copy */
int td_qwen2_read_kv(td_qwen2* f, int layer, int slot, int row0, int n, void* out_bf16, void* stream);
/* kv bf16 [rows, ld] with `heads` 128-wide head vectors per row -> bytes at q[dst, h 128 ..] (ldq BYTES per row) and 2^e at scale[dst, h] (lds floats per
 * row), dst = dst_rows[r] (device int32[rows]) or r when NULL; kv_hat (NULL, or bf16 [rows, ld]; may alias kv) receives x^ at row r.  ld % 8 == 0,
 * ldq % 8 == 0, both >= heads x 128, lds >= heads; kv / kv_hat 16-byte, q 8-byte, scale / dst_rows 4-byte aligned.  A NULL kv / q / scale, rows or
 * heads <= 0, a bad stride or a misaligned pointer: TD_ERR_INVALID with a message, before any HIP call.  Rows named by nobody are not touched. */
int td_kv_quant_rows_e4m3(const void* kv, int64_t ld, void* q, int64_t ldq, float* scale, int64_t lds, void* kv_hat,
                          int rows, int heads, const int* dst_rows, void* stream);
/* ... and back: out[r, h 128 + d] = q[r, h 128 + d] scale[r, h] as bf16 (exact).  The same rules. */
int td_kv_dequant_rows_e4m3(const void* q, int64_t ldq, const float* scale, int64_t lds, void* out, int64_t ld, int rows, int heads, void* stream);
/* Decode attention (one query token per sequence, td_attention_bf16 with Sq = 1 and causal) over an e4m3 cache: q [batch][1, Hq 128] bf16 (q_bstride
 * elements apart), k8 / v8 [batch][Skv, ldkv] bytes (ldkv and kv_bstride in BYTES; head h at byte h 128), k_scale / v_scale [batch][Skv, lds] fp32 (head h at
 * column h; s_bstride floats apart), o as q.  Sequence b attends keys [0, kv_lens[b]) (device int32[batch]), or all Skv when NULL.
 * td_attention_decode_set_group governs this form too.  ldkv % 8 == 0, kv_bstride % 8 == 0, q / o 16-byte, k8 / v8 8-byte, scales 4-byte aligned; a NULL
 * operand, a bad stride or a misaligned pointer: TD_ERR_INVALID with a message, before any HIP call. */
int td_attention_decode_kv8(const void* q, int64_t ldq, int64_t q_bstride, const void* k8, const void* v8, int64_t ldkv, int64_t kv_bstride,
                            const float* k_scale, const float* v_scale, int64_t lds, int64_t s_bstride, void* o, int64_t ldo, int64_t o_bstride,
                            int batch, int Skv, const int* kv_lens, int Hq, int Hkv, float scale, void* stream);

/* Qwen2 building blocks */
/* out bf16[n,D] = table[ids[i],:] (table bf16 [vocab,D], ids device int32[n], D % 8 == 0).  An id outside [0, vocab) is CLAMPED, not
 * refused: id < 0 reads row 0, id >= vocab reads row vocab - 1 (the kernel never reads outside the table; a caller that wants an
 * error for a bad id checks on the host). */
int td_embed_gather_bf16(const int* ids, const void* table, void* out, int n, int D, int vocab, void* stream);
int td_silu_mul_bf16(const void* gate_up, void* out, int rows, int I, void* stream);
/* M-RoPE tables: pos3n device int32 [3,n] (temporal, height, width), sections3 HOST ints summing to 64; cos/sin fp32 [n,128], column j and
 * 64 + j = cosf/sinf(float(pos[axis(j)]) * inv_freq_j), inv_freq_j = 1.0f / fp32(theta^(2j/128)) with the power correctly rounded (the
 * arithmetic of Qwen2VLRotaryEmbedding in fp32), axis(j) = the section j falls in; round_bf16: values rounded to bf16. */
int td_mrope_table(const int* pos3n, int n, const int* sections3, float theta, int round_bf16, float* cos, float* sin, void* stream);
/* Temperature / top-p (nucleus) sampling, one token per row of bf16 logits [rows, ld], in ONE launch and without a sort:
 *   p = softmax(logits / temperature); keep the most likely tokens while the mass in front of a token is < top_p; renormalise;
 *   draw one token per row -> out_ids[rows] (device int32).  temperature <= 0: greedy (first index of the row maximum).
 * The draw of row r is a pure function of (seed, offset, r): callers advance `offset` once per generated token.
 * vocab % 8 == 0, ld % 8 == 0, rows <= 65535.  Replaces the sampler of vllm.SamplingParams(temperature, top_p) inside
 * LLM.generate (thinkdiff/models/mllama_vllm_t5_embed_decoder_2.py:817-823, thinkdiff/models/mllama_vllm_generate_1.py:398-405). */
int td_sample_top_p_bf16(const void* logits, int64_t ld, int rows, int vocab, float temperature, float top_p,
                         uint64_t seed, uint64_t offset, int32_t* out_ids, void* stream);

/* ---- per-request sampler (td_abi_version() >= 14): top-k, top-p, min-p and the three penalties, every value per row ----
 * The rest of what a caller sets on vllm.SamplingParams per prompt ([ext] vLLM sampler: apply_penalties, _apply_top_k_top_p, _apply_min_p), in ONE
 * launch without a sort.  For a row with bf16 logits x[0..vocab), prompt token set P and generated-token counts c[t] (both from the row's slot):
 *   z[t] = float(x[t]);  for t in P or c[t] > 0:  z[t] = z[t] > 0 ? z[t] / repetition_penalty : z[t] * repetition_penalty;
 *          z[t] -= frequency_penalty * c[t];  z[t] -= presence_penalty * (c[t] > 0)            (fp32, never rounded back to bf16)
 *   temperature <= 0: the first index holding max z.  Otherwise p = softmax(z / temperature) and the kept set is the intersection of
 *     top-k   the k most likely tokens (off when top_k <= 0 or top_k >= vocab),
 *     top-p   of the top-k set: a token is kept iff the mass in front of it is < top_p x (top-k mass)  (td_sample_top_p_bf16's rule),
 *     min-p   z[t] >= max z + temperature x ln(min_p), i.e. p[t] >= min_p x max p (off when min_p <= 0);
 *   renormalise, draw one token.  Ties at a boundary resolve in index order of the kernel's walk (any tied token, the count the rule gives).
 * The draw is td_sample_top_p_bf16's function of (seed, offset, stream) with `stream` in the place of its row number: rows with one seed and
 * offset, stream = row, slot = -1 and every filter off return td_sample_top_p_bf16's ids bit for bit.
 * Out-of-range per-row values never fault: top_p <= 0 keeps the top token only, top_p > 1 or NaN is 1; min_p > 1 is 1; repetition_penalty <= 0 or
 * non-finite is 1; a non-finite presence / frequency penalty is 0; slot outside [0, n_slots) is "no history".  Degenerate rows as
 * td_sample_top_p_bf16, after the penalties: a +inf value wins (first index), a row of -inf / NaN yields id 0, one finite value is always taken. */
typedef struct TdSampleRow {
  float temperature, top_p, min_p, repetition_penalty, presence_penalty, frequency_penalty;
  int top_k;
  int slot;        /* history slot of the td_sampler, -1: no history */
  int stream;      /* the draw's third key (td_sample_top_p_bf16's row number) */
  uint64_t seed;
} TdSampleRow;
size_t td_sample_row_size(void);      /* sizeof(TdSampleRow), for bindings that restate the struct */

/* Token history of n_slots sequences over one vocabulary: per slot a prompt-presence bitmap, a bitmap of the tokens with history (prompt or
 * generated) and a uint16 count per vocabulary entry, exact to 65 535 and saturating there: n_slots x vocab x 2.25 bytes of device memory
 * (87.6 MB at 256 x 152 064), allocated here and zeroed.  n_slots 1..65535, vocab % 8 == 0. */
typedef struct td_sampler td_sampler;
int td_sampler_create(int n_slots, int vocab, td_sampler** out);
void td_sampler_destroy(td_sampler* s);
/* Clear a slot and mark prompt_ids_dev[0..n_prompt) (device int32; ids outside [0, vocab) are ignored; n_prompt 0 with a NULL pointer just clears). */
int td_sampler_reset_slot(td_sampler* s, int slot, const int* prompt_ids_dev, int n_prompt, void* stream);
/* Tests and debugging: counts as int32 [vocab], the prompt set as uint8 [vocab] (0 / 1); set_counts replaces the counts (clamped to 0..65535) and
 * rebuilds the slot's history bitmap from them and the prompt bitmap. */
int td_sampler_read_counts(const td_sampler* s, int slot, int32_t* out_dev, void* stream);
int td_sampler_read_prompt_mask(const td_sampler* s, int slot, uint8_t* out_dev, void* stream);
int td_sampler_set_counts(td_sampler* s, int slot, const int32_t* counts_dev, void* stream);
/* One token per row -> out_ids[rows].  params_dev: rows TdSampleRow structs, offsets_dev: rows int64 (the draw's second key, per row), both in
 * device memory.  s may be NULL iff every row has slot == -1 (the caller's promise: the kernel reads no history when s is NULL).
 * update_state = 1: the thread that writes out_ids[row] also adds 1 to the slot's count of that token (saturating) and marks it in the history
 * bitmap; the slots named by one launch must then be distinct (not checked: two rows on one slot race on its counts).  update_state = 0: the
 * state is only read and rows may share a slot.  TD_ERR_INVALID before any HIP call: a NULL logits / params / offsets / out_ids; vocab % 8,
 * ld % 8 or logits not 16-byte aligned; rows outside 1..65535; vocab != the state's; update_state with s == NULL. */
int td_sample_rows_bf16(const td_sampler* s, const void* logits, int64_t ld, int rows, int vocab, const TdSampleRow* params_dev,
                        const int64_t* offsets_dev, int update_state, int32_t* out_ids, void* stream);

/* ---- logit edits in the sampler's launch (td_abi_version() >= 15): logit_bias, allowed_token_ids, bad words and the min_tokens stop mask of
 * vllm.SamplingParams ([ext] vLLM V1 sampler: allowed ids, then bad words, then min-tokens and logit bias, then penalties), as one per-row edit
 * of the logits in front of the penalties.  For a row with bf16 logits x, an edit slot (banned set B, bias b) and the history above:
 *   z[t] = -inf                   if t in B              (a banned token stays banned whatever its bias)
 *   z[t] = float(x[t]) + b[t]     if t has a bias        (fp32, never rounded back to bf16; NaN -> -inf, so a -inf logit with a +inf bias is -inf)
 *   z[t] = float(x[t])            otherwise              (NaN -> -inf, as above)
 * then the penalties of td_sample_rows_bf16 on z (the repetition sign test sees the biased value), then temperature, top-k, top-p, min-p and the
 * draw, unchanged.  A row whose every token is banned is a row of -inf: id 0, never a fault.
 * State: n_slots edit slots over one vocabulary; per slot a ban bitmap and a bias bitmap (one byte of each per 8 tokens, read beside the logits;
 * the kernel reads both rather than their OR, so that an edited chunk costs no second, dependent read) and a table of at most TD_MAX_LOGIT_BIAS
 * (token, fp32 value) pairs sorted by token, which a workgroup stages in LDS and searches for biased tokens only:
 * n_slots x (2 x vocab / 8 + 8 x TD_MAX_LOGIT_BIAS + 4) bytes of device memory, 11.8 MB at 256 x 152 064, allocated here and zeroed.
 * Every setter is stream-ordered, makes no allocation and no host synchronisation, and refuses a NULL state or a slot outside [0, n_slots) with
 * TD_ERR_INVALID before any HIP call. */
#define TD_MAX_LOGIT_BIAS 1024
typedef struct td_logit_edits td_logit_edits;
int td_logit_edits_create(int n_slots, int vocab, td_logit_edits** out);      /* n_slots 1..65535, vocab % 8 == 0 */
void td_logit_edits_destroy(td_logit_edits* e);
/* Clear the slot's bans and biases. */
int td_logit_edits_reset_slot(td_logit_edits* e, int slot, void* stream);
/* Replace the slot's bias table.  ids / values are HOST arrays of n entries, read before the call returns (the library sorts them and hands them to
 * the device in the launches' arguments).  Refused before any HIP call: n > TD_MAX_LOGIT_BIAS, an id given twice, an id outside [0, vocab).
 * A NaN value counts as 0; +-inf is honoured.  n = 0 clears the table. */
int td_logit_edits_set_bias(td_logit_edits* e, int slot, const int32_t* ids, const float* values, int n, void* stream);
/* Set (on != 0) or clear the ban on ids_dev[0..n) (DEVICE int32; ids outside the vocabulary are ignored).  Clearing a ban restores the token's
 * bias if it has one. */
int td_logit_edits_ban(td_logit_edits* e, int slot, const int32_t* ids_dev, int n, int on, void* stream);
/* Ban every token except ids_dev[0..n) (DEVICE int32; ids outside the vocabulary are ignored; replaces the slot's bans, keeps its biases). */
int td_logit_edits_allow_only(td_logit_edits* e, int slot, const int32_t* ids_dev, int n, void* stream);
/* Tests and debugging: the banned set as uint8 [vocab] (0 / 1) and the biases as fp32 [vocab] (0 where none), device memory; either may be NULL. */
int td_logit_edits_read(const td_logit_edits* e, int slot, uint8_t* banned_u8_out_dev, float* bias_f32_out_dev, void* stream);
/* td_sample_rows_bf16 with the edits of slot edit_slots_dev[row] applied to row `row` (device int32 [rows]; -1 or any value outside [0, n_slots):
 * no edits for that row).  The launch only reads the edit state, so rows may share an edit slot.  e == NULL: the call IS td_sample_rows_bf16
 * (edit_slots_dev is not read); a row without edits returns td_sample_rows_bf16's id bit for bit.  TD_ERR_INVALID before any HIP call: what
 * td_sample_rows_bf16 refuses, a NULL edit_slots_dev with e set, vocab != the edit state's. */
int td_sample_rows_edit_bf16(const td_sampler* s, const td_logit_edits* e, const int32_t* edit_slots_dev, const void* logits, int64_t ld, int rows,
                             int vocab, const TdSampleRow* params_dev, const int64_t* offsets_dev, int update_state, int32_t* out_ids, void* stream);

/* ---- logprobs of rows of bf16 logits (td_abi_version() >= 15; csrc/logprobs_rows.hip), one workgroup per row, no sort ----
 * Takes the RAW logits, before edits, penalties and temperature (vLLM V1's default logprobs mode, `raw_logprobs`).  Per row:
 *   m = max x,  lse = m + ln(sum exp(x - m)),  lp[t] = float(x[t]) - lse
 * with the sum taken over 2^-40 fixed-point masses in 64-bit integers, so it does not depend on the order of accumulation: one row gives the same
 * bits at any row index and row count.
 *   ids_dev[rows]     the sampled or forced token of each row;
 *   n_top_dev[rows]   < 0: the row is skipped and its outputs are left untouched; 0: the chosen token only; up to top_cap (larger: top_cap);
 *   lp_sampled[rows]  fp32, the chosen token's logprob;       rank[rows]  int32, the number of t with x[t] >= x[id] (vLLM's batched_count_greater_than);
 *   top_ids / top_lp  [rows, top_cap] int32 / fp32: the n_top largest logits in descending value, then ascending index (ties go to the lower index),
 *                     found with the 16-bit radix select of td_sample_top_p_bf16; unused columns hold id -1 and lp -inf.
 * Degenerate rows never fault and no output is ever NaN -- where torch.log_softmax returns NaN, this does not: a NaN logit counts as -inf; a row
 * with no finite value and no +inf gives lp -inf for every token and rank = vocab; in a row holding +inf those tokens get lp 0 and every other
 * token -inf; an id outside [0, vocab) gives lp -inf and rank 0.
 * vocab % 8 == 0, ld % 8 == 0, ld >= vocab, rows 1..65535, 0 <= top_cap <= TD_MAX_LOGPROBS (top_ids / top_lp may be NULL iff top_cap == 0), logits
 * 16-byte aligned; TD_ERR_INVALID before any HIP call otherwise. */
#define TD_MAX_LOGPROBS 20
int td_logprobs_rows_bf16(const void* logits, int64_t ld, int rows, int vocab, const int32_t* ids_dev, const int32_t* n_top_dev, int top_cap,
                          float* lp_sampled, int32_t* rank, int32_t* top_ids, float* top_lp, void* stream);

/* ---- beam search: the step's choice and placement on the device (td_abi_version() >= 18; csrc/beam_search.hip), one wave per request ----
 * A launch covers R requests of W rows each; row r*W + j is cache-slot position j of request r.  n_in (HOST) = 1 at the first step, when only row
 * r*W of a request is live (it holds the prefill), W afterwards.  Inputs (device): top_ids int32 / top_lp fp32 [R*W, cap], cap >= 2W -- what
 * td_logprobs_rows_bf16 returns with n_top = 2W; cum_in fp32 [R*W]; rank_in int32 [R*W], the rank of the beam living in each row; eos: a token id,
 * or -1 for none.  The rule, per request:
 *   a candidate is (live row j, column c < 2W) with id >= 0 and cum = cum_in[j] + top_lp[j][c] (ONE fp32 add; a NaN sum counts as -inf);
 *   id == eos: a FINISHER of row j -- fin_flag[j] = 1, fin_cum[j] = cum (the first such column) -- and not a beam candidate; rows without one get
 *   fin_flag 0 and fin_cum -inf;
 *   the other candidates in the order (cum descending, rank_in ascending, c ascending[, j ascending]): the first W are the new beams, ranks 0..W-1;
 *   with fewer than W candidates the missing beams have token -1, cum -inf and no parent.
 * Slot-stable placement: walking the new beams in rank order, a beam whose parent's row is not yet claimed takes that row (no copy); the remaining
 * beams, in rank order, take the unclaimed rows in ascending order and get copy_src = the absolute row index of their parent.  So every source row
 * keeps its own beam, every destination is the row of a beam that died, and td_kv_gather_rows can do all copies of the step in one call.
 * Outputs per row (device, [R*W]; the caller passes per-step slices of [T, R*W] logs and reads a generation back once): token, cum_out, rank_out,
 * copy_src (-1: no copy), parent (absolute row of the parent; the own row for a missing beam), fin_flag, fin_cum.  Nothing faults and no output
 * is NaN.  TD_ERR_INVALID with a message naming the value, before any HIP call: a NULL pointer, W outside 1..TD_MAX_BEAM_WIDTH (2W must fit
 * TD_MAX_LOGPROBS), cap < 2W, n_in not in {1, W}, R < 1, R*W > 65535. */
#define TD_MAX_BEAM_WIDTH 10
int td_beam_select(const int32_t* top_ids, const float* top_lp, int cap, const float* cum_in, const int32_t* rank_in, int R, int W, int n_in, int eos,
                   int32_t* token, float* cum_out, int32_t* rank_out, int32_t* copy_src, int32_t* parent, int32_t* fin_flag, float* fin_cum, void* stream);

/* ---- speculative decoding: a multi-row verify step and the accept rule (td_abi_version() >= 21) ----
 * Multi-row decode attention (csrc/attention_decode.hip).  Sequence b of n_seq (1..256) owns the query rows [seq_row0[b], seq_row0[b] + seq_rows[b]) of
 * q / o (row strides ldq / ldo, elements), 1 <= seq_rows[b] <= TD_MAX_VERIFY_ROWS; row j of it sees keys [0, seq_len0[b] + j) of cache slot seq_slot[b]
 * (slot stride kv_bstride; s_bstride for the scales).  seq_len0[b] counts the keys visible to the first row, that row's own key included; the new rows'
 * k | v are in the cache when the launch starts.  bf16 cache: k, v set (ldkv, kv_bstride in elements), k8 / v8 / k_scale / v_scale NULL; e4m3 cache
 * (the format of td_kv_quant_rows_e4m3): k8, v8, k_scale, v_scale set (ldkv, kv_bstride in bytes; lds, s_bstride in floats), k / v NULL.
 * Two forms.  Form 1, one workgroup per (q-head group, row): the single-row kernel's own body, K/V read once per row; row (b, j) receives the BITS
 * td_attention_bf16 (Sq = 1, causal) / td_attention_decode_kv8 give one query with kv_lens = seq_len0[b] + j on the same cache under the same q-head group.
 * Form 2, one workgroup per (q-head group, sequence, chunk of T rows): K/V read once for the G x T <= 8 (row, head) states of a workgroup; its softmax
 * update is written out as fmas, so its result is the same under every G and T but differs from form 1 in the last bf16 bit of a fraction of a per cent of
 * the rows: it is held to one bf16 ulp + 2^-12 max |v| of the float64 result, not to bit equality.  The automatic routing (td_attention_verify_set_form:
 * 0 = automatic, 1, 2; returns the previous value; tests and A/B) takes form 2 only where it measured faster -- 2 .. 4 rows per sequence with
 * Hq x n_seq below the CU count, on the e4m3 cache or from 4096 keys on -- which it can only know through td_attention_verify_ex: this entry always runs
 * form 1 unless forced.  td_attention_decode_set_group forces G in both forms.
 * The four per-sequence arrays are DEVICE int32, so their values cannot be checked on the host: the kernels clamp seq_rows[b] to 1..TD_MAX_VERIFY_ROWS and
 * never read a key at or past seq_len0[b] + seq_rows[b] - 1.
 * TD_ERR_INVALID with a message naming the value, before any HIP call: a NULL operand, both or neither cache form, n_seq outside 1..256, Hq % Hkv != 0,
 * ldq / ldo / ldkv / kv_bstride not multiples of 8 or narrower than their heads, q / o / k / v not 16-byte, k8 / v8 not 8-byte, scales or arrays not
 * 4-byte aligned. */
#define TD_MAX_VERIFY_ROWS 8
int td_attention_verify(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, int64_t kv_bstride, const void* k8, const void* v8,
                        const float* k_scale, const float* v_scale, int64_t lds, int64_t s_bstride, void* o, int64_t ldo, int n_seq,
                        const int32_t* seq_row0_dev, const int32_t* seq_rows_dev, const int32_t* seq_len0_dev, const int32_t* seq_slot_dev, int Hq, int Hkv,
                        float scale, void* stream);
int td_attention_verify_set_form(int form);
/* ... for a caller that knows on the HOST what the device arrays hold: t_max = the largest seq_rows[b] (1..8; seq_rows[b] is clamped to it, and the grid
 * is laid out for it), max_len = the longest visible length seq_len0[b] + seq_rows[b] - 1 (0 = unknown; it only feeds the automatic routing).
 * td_attention_verify is this entry with t_max = 8 and max_len = 0.  Stateless: nothing a call passes here outlives it. */
int td_attention_verify_ex(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, int64_t kv_bstride, const void* k8, const void* v8,
                           const float* k_scale, const float* v_scale, int64_t lds, int64_t s_bstride, void* o, int64_t ldo, int n_seq,
                           const int32_t* seq_row0_dev, const int32_t* seq_rows_dev, const int32_t* seq_len0_dev, const int32_t* seq_slot_dev, int Hq, int Hkv,
                           float scale, int t_max, int max_len, void* stream);

/* The verify step of the Qwen2-VL engine: sequence b (cache slot slots[b], HOST ints, distinct; NULL = 0 .. B-1) feeds n_new[b] tokens (HOST, 1..8) at
 * cache rows cache_pos[b] .. (HOST).  R = sum n_new <= 256 rows, sequence after sequence: token_ids int32[R], position_ids int32[3, R] (device);
 * hidden_out bf16[R, hidden], logits bf16[R, vocab] (either may be NULL).  Row (b, j) is what td_qwen2_decode_batch_slots returns for that token had the
 * j tokens before it been decoded one step at a time (the same launches under the routing a step of R sequences takes; always the separate rotary +
 * cache-write launch, then td_attention_verify's kernels).  The call runs eagerly; with every n_new == 1 it IS td_qwen2_decode_batch_slots.
 * No rollback: all R new k | v rows are written; a caller that rejects tokens advances cache_pos by what it keeps and the next step overwrites the rest.
 * TD_ERR_INVALID before any launch: what td_qwen2_decode_batch_slots refuses, n_new[b] outside 1..8, cache_pos[b] + n_new[b] > the slot capacity,
 * R above 256 or above the workspace rows. */
int td_qwen2_verify_batch_slots(td_qwen2* f, int B, const int* slots, const int* n_new, const int* token_ids, const int* position_ids, const int* cache_pos,
                                void* hidden_out, void* logits, void* stream);

/* The accept rule (csrc/spec_decode.hip).  sampled[r] = the token SAMPLED from row r's logits, input[r] = the token that was fed as row r (device
 * int32[R]); sequence b owns rows [seq_row0[b], seq_row0[b] + seq_rows[b]) (device int32[B], seq_rows clamped to 1..TD_MAX_VERIFY_ROWS).
 *   a[b] = the number of leading j < seq_rows[b] - 1 with input[row0 + j + 1] == sampled[row0 + j];
 *   n_emit[b] = a[b] + 1;  emit[b, 0 .. a[b]] = sampled[row0 .. row0 + a[b]], the other columns of emit int32[B, TD_MAX_VERIFY_ROWS] hold -1.
 * Every emitted token is a draw from the target distribution on a true prefix; the guesses decide only how many rows were.
 * TD_ERR_INVALID before any HIP call: a NULL or misaligned pointer, B outside 1..256. */
int td_spec_accept(const int32_t* sampled_dev, const int32_t* input_dev, const int32_t* seq_row0_dev, const int32_t* seq_rows_dev, int B,
                   int32_t* n_emit_dev, int32_t* emit_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* THINKDIFF_HIP_H */
