// extern "C" surface of libthinkdiff_hip.so (declared in include/thinkdiff_hip.h).
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include "td_kernels.h"
#include "../../include/thinkdiff_hip.h"

static thread_local char g_err[512] = "";

void td_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" {

const char* td_last_error(void) { return g_err; }
int td_abi_version(void) { return 26; }  // 2: TdFluxConfig::out_channels appended (channel-conditioned FLUX); 3: LoRA adapters, td_flux_read_param;
                                            // 4: FLUX ControlNet (td_flux_controlnet_*, td_flux_attach_controlnet, td_flux_residual_inject_bf16)
                                            // 5: FLUX IP-Adapter (td_ip_attention_bf16, td_flux_ip_adapter_*, td_flux_set_ip_image_embeds)
                                            // 6: first-block cache (td_block_cache_*_bf16, td_flux_set_block_cache*, td_flux_block_cache_*)
                                            // 7: int8 policy building blocks (td_norm_rows_quant8, td_quant_rows8, td_col_amax_bf16, td_smooth_factors,
                                            //    td_q8_scales_from_amax, td_ext_cols_int8, td_linear*_int8_q8, td_attention_q8, td_attention_fp8_q8)
                                            // 8: FLUX.1 Redux (td_abi_version() >= 8: td_redux_compose_bf16)
                                            // 9: td_linear_drain_bf16 (test entry of the 256x256 tile's persistent walk)
                                            // 10: several ControlNets per context (td_flux_attach_controlnets, td_flux_set_controlnet_scales_at,
                                            //     td_flux_attached_controlnets, td_flux_residual_inject_multi_bf16)
                                            // 11: PIL-exact image resize (td_resize_coeffs, td_image_resize_u8, td_image_lut_chw_f32)
                                            // 12: 8-bit weight stream (td_quant_weight_rows_e4m3, td_linear*_w8_bf16, td_linear_glu_bf16,
                                            //     td_qwen2_quantize_weights, td_qwen2_set_weight_stream, td_qwen2_weight_info, td_qwen2_weight_stream_launches)
                                            // 13: e4m3 KV cache (td_qwen2_create_kv, td_qwen2_kv_info, td_qwen2_read_kv, td_kv_quant_rows_e4m3,
                                            //     td_kv_dequant_rows_e4m3, td_attention_decode_kv8)
                                            // 14: per-request sampler (td_sampler_*, td_sample_rows_bf16, td_sample_row_size; csrc/sampler_rows.hip)
                                            // 15: logit edits in the sampler's launch (td_logit_edits_*, td_sample_rows_edit_bf16) and logprobs
                                            //     (td_logprobs_rows_bf16; csrc/logprobs_rows.hip)
                                            // 16: KV fork (td_kv_fork_rows, td_qwen2_fork_slot; csrc/kv_fork.hip)
                                            // 17: td_attention_segments_bf16 (packed segments with a causal switch: the packed prefill's launch);
                                            //     td_softmax_rows_* refuse a scale that is not finite and positive
                                            // 18: beam search (td_beam_select; csrc/beam_search.hip) and the KV gather behind it (td_kv_gather_rows,
                                            //     td_qwen2_gather_slots; csrc/kv_fork.hip)
                                            // 19: td_gemm_plan_query (host-only: the tile an automatic GEMM launch takes, alone or on a shared chip)
                                            // 20: MXFP4 weight stream (td_quant_weight_rows_mxfp4, td_dequant_rows_mxfp4, td_linear*_w4_bf16,
                                            //     TD_QWEN2_WEIGHTS_MXFP4)
                                            // 21: speculative decoding (td_attention_verify, td_attention_verify_ex, td_attention_verify_set_form,
                                            //     td_qwen2_verify_batch_slots, td_spec_accept; csrc/spec_decode.hip)
                                            // 22: grouped int4 weight stream for AWQ / GPTQ checkpoints (td_repack_int4, td_dequant_rows_int4,
                                            //     td_linear*_i4_bf16, td_qwen2_load_param_int4, td_qwen2_set_int4_routing, TD_QWEN2_WEIGHTS_INT4)
                                            // 23: prefix caching (td_attention_prefix_segments_bf16: packed query segments over key ranges of their own;
                                            //     td_qwen2_prefill_packed_prefix_slots: the packed prefill behind cached prefixes)
                                            // 24: per-request LoRA (td_lora_rows_bf16, td_lora_rows_pack_bf16: the row-indexed low-rank add,
                                            //     csrc/lora_rows.hip; td_qwen2_lora_*: the adapter pool of the Qwen2-VL decode engine)
                                            // 25: the FLUX step's row kernels alone (td_qk_norm_rope_premul_bf16, td_temb_combine_silu_bf16,
                                            //     td_copy_cols_bf16, td_fill_normal_from_bf16: test entries of launches only the engines made)
                                            // 26: the VAE decoder's boundary kernels alone (td_vae_latents_to_nhwc_bf16, td_vae_image_finalize: test
                                            //     entries of the two launches only td_vae_decode made)

int td_linear_bf16(const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy,
                   int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr,
                   void* stream) {
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx;
  p.W = (const bf16_t*)w; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y; p.ldc = (int)ldy;
  p.gate = (const bf16_t*)gate; p.res = (const bf16_t*)res; p.ldr = (int)ldr;
  p.M = M; p.N = N; p.K = K; p.act = act;
  return td_gemm_launch(p, (hipStream_t)stream);
}

int td_linear_split_bf16(const void* x, int64_t ldx, const void* w, const void* bias,
                         void* y0, int64_t ldy0, int act0, void* y1, int64_t ldy1, int act1,
                         int M, int N, int K, int n_split, void* stream) {
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx;
  p.W = (const bf16_t*)w; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y0; p.ldc = (int)ldy0; p.act = act0;
  p.C2 = (bf16_t*)y1; p.ldc2 = (int)ldy1; p.act2 = act1; p.n_split = n_split;
  p.M = M; p.N = N; p.K = K;
  return td_gemm_launch(p, (hipStream_t)stream);
}

int td_linear_splitk_bf16(const void* x, int64_t ldx, const void* w, const void* bias, void* y0, int64_t ldy0, void* y1, int64_t ldy1, int n_split,
                          int M, int N, int K, const void* res, int64_t ldr, int tile_cfg, int split_k,
                          const void* norm_w, void* norm_out, int64_t ld_norm, float norm_eps, void* stream) {
  TdGemmParams p;
  p.sk_norm_w = (const bf16_t*)norm_w; p.sk_norm_out = (bf16_t*)norm_out; p.sk_norm_ld = (int)ld_norm; p.sk_norm_eps = norm_eps;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W = (const bf16_t*)w; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y0; p.ldc = (int)ldy0; p.C2 = (bf16_t*)y1; p.ldc2 = (int)ldy1; p.n_split = y1 ? n_split : 0;
  p.res = (const bf16_t*)res; p.ldr = (int)ldr; p.M = M; p.N = N; p.K = K; p.cfg = tile_cfg; p.split_k = split_k;
  return td_gemm_launch(p, (hipStream_t)stream);
}

int td_linear_grouped2_bf16(const void* x0, int M0, const void* w0, const void* bias0, const void* gate0,
                            const void* res0, void* y0, const void* x1, int M1, const void* w1,
                            const void* bias1, const void* gate1, const void* res1, void* y1,
                            int64_t ldx, int64_t ldy, int64_t ldr, int N, int K, int act, int tile_cfg,
                            void* stream) {
  TdGemmParams p;
  p.A = (const bf16_t*)x0; p.W = (const bf16_t*)w0; p.bias = (const bf16_t*)bias0; p.gate = (const bf16_t*)gate0;
  p.res = (const bf16_t*)res0; p.C = (bf16_t*)y0; p.M = M0;
  p.g_A = (const bf16_t*)x1; p.g_W = (const bf16_t*)w1; p.g_bias = (const bf16_t*)bias1; p.g_gate = (const bf16_t*)gate1;
  p.g_res = (const bf16_t*)res1; p.g_C = (bf16_t*)y1; p.g_M = M1;
  p.lda = (int)ldx; p.ldc = (int)ldy; p.ldr = (int)ldr; p.N = N; p.K = K; p.act = act; p.cfg = tile_cfg;
  return td_gemm_launch(p, (hipStream_t)stream);
}

int td_gemm_plan_query(int M, int N, int K, int shared, int operand) {
  if (M < 1 || N < 1 || K < 1 || operand < TD_OPERAND_BF16 || operand > TD_OPERAND_E4M3) {
    td_set_error("td_gemm_plan_query: M=%d N=%d K=%d must be positive and operand=%d one of 0 (bf16), 1 (int8), 2 (e4m3)", M, N, K, operand);
    return -1;
  }
  return td_gemm_plan(M, N, operand == TD_OPERAND_BF16 ? K : K / 2, shared, operand);      // (8-bit operands: tiles are chosen by bytes, as td_gemm_launch does)
}

int td_linear_drain_bf16(const void* x0, int M0, const void* w0, const void* bias0, const void* gate0, const void* res0, void* y0,
                         const void* x1, int M1, const void* w1, const void* bias1, const void* gate1, const void* res1, void* y1,
                         int64_t ldx, int64_t ldy, int64_t ldr, int N, int K, int act,
                         void* y_split, int64_t ld_split, int act_split, int n_split, int max_workgroups, void* stream) {
  TD_CHECK_ARG(max_workgroups >= 0, "td_linear_drain_bf16: max_workgroups=%d must not be negative", max_workgroups);
  TdGemmParams p;
  p.A = (const bf16_t*)x0; p.W = (const bf16_t*)w0; p.bias = (const bf16_t*)bias0; p.gate = (const bf16_t*)gate0;
  p.res = (const bf16_t*)res0; p.C = (bf16_t*)y0; p.M = M0;
  p.g_A = (const bf16_t*)x1; p.g_W = (const bf16_t*)w1; p.g_bias = (const bf16_t*)bias1; p.g_gate = (const bf16_t*)gate1;
  p.g_res = (const bf16_t*)res1; p.g_C = (bf16_t*)y1; p.g_M = x1 ? M1 : 0;
  p.lda = (int)ldx; p.ldc = (int)ldy; p.ldr = (int)ldr; p.N = N; p.K = K; p.act = act;
  p.C2 = (bf16_t*)y_split; p.ldc2 = (int)ld_split; p.act2 = y_split ? act_split : TD_ACT_NONE; p.n_split = y_split ? n_split : 0;
  p.cfg = 0; p.drain_cap = max_workgroups;
  return td_gemm_launch(p, (hipStream_t)stream);
}

int td_conv3x3_nhwc_bf16(const void* x, const void* w, const void* bias, const void* res, void* y,
                         int H, int W, int Cin, int Cout, int upsample2x, void* stream) {
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = Cin; p.W = (const bf16_t*)w; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y; p.ldc = Cout; p.res = (const bf16_t*)res; p.ldr = Cout;
  p.M = H * W; p.N = Cout; p.K = 9 * Cin;
  p.conv_H = H; p.conv_W = W; p.conv_Cin = Cin; p.conv_up = upsample2x ? 1 : 0;
  return td_gemm_launch(p, (hipStream_t)stream);
}

int td_linear_f32out_bf16(const void* x, int64_t ldx, const void* w, const void* bias, float* y, int64_t ldy,
                          int M, int N, int K, void* stream) {
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W = (const bf16_t*)w; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y; p.ldc = (int)ldy; p.M = M; p.N = N; p.K = K; p.out_f32 = 1; p.cfg = (N <= 64) ? 1 : (M <= 32 ? 2 : 0);
  return td_gemm_launch(p, (hipStream_t)stream);
}

static int g_attn_variant = 0;
int td_attention_set_variant(int variant) {
  const int prev = g_attn_variant;
  g_attn_variant = variant;
  return prev;
}

int td_attention_bf16(const void* q, int64_t ldq, int64_t q_bstride, const void* k, const void* v,
                      int64_t ldkv, int64_t kv_bstride, void* o, int64_t ldo, int64_t o_bstride,
                      int batch, int Sq, int Skv, int Hq, int Hkv, int head_dim, float scale,
                      int causal, void* stream) {
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)o;
  p.batch = batch; p.Sq = Sq; p.Skv = Skv; p.Hq = Hq; p.Hkv = Hkv; p.head_dim = head_dim;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo;
  p.q_bstride = q_bstride; p.kv_bstride = kv_bstride; p.o_bstride = o_bstride;
  p.scale = scale; p.causal = causal; p.causal_offset = Skv - Sq; p.variant = g_attn_variant & ~0x800;
  // test hook (td_attention_set_variant bit 0x800): q already carries scale * log2(e) -- the form the FLUX engine's RoPE kernel hands over
  p.q_prescaled = (g_attn_variant & 0x800) && !causal ? 1 : 0;
  return td_attn_launch(p, (hipStream_t)stream);
}

int td_attention_joint_prescaled_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo, int S, int H, float score_bound, void* stream) {
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)o;
  p.batch = 1; p.Sq = S; p.Skv = S; p.Hq = H; p.Hkv = H; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo; p.scale = 1.0f; p.causal = 0; p.causal_offset = 0; p.variant = g_attn_variant & 0x4ff;      // (bit 0x400: the 32x32x16 body, A/B)
  p.q_prescaled = 1; p.score_bound = score_bound;
  return td_attn_launch(p, (hipStream_t)stream);
}

size_t td_attention_fp8_workspace_bytes(int Sq, int Skv, int Hq) { return Sq > 0 && Skv > 0 && Hq > 0 ? td_attn_fp8_ws_bytes(Sq, Skv, Hq) : 0; }

int td_attention_fp8(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo,
                     int Sq, int Skv, int Hq, float scale, void* workspace, void* stream) {
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)o;
  p.batch = 1; p.Sq = Sq; p.Skv = Skv; p.Hq = Hq; p.Hkv = Hq; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo; p.scale = scale; p.f8_ws = workspace; p.variant = ((g_attn_variant & 1) ? 0x1000 : 0) | ((g_attn_variant & 2) ? 0x2000 : 0) | (((g_attn_variant >> 4) & 7) << 16);      // td_attention_set_variant bit 0: the 4-wave A/B form, bit 1: exp2 probabilities, bits 4-6: timing-only probes (TD_ATTN8_PROBE builds)
  return td_attn_fp8_launch(p, (hipStream_t)stream);
}

int td_attention_fp8_qk_rope(const void* qkv, int64_t ld, int q_col, int k_col, int v_col, void* o, int64_t ldo, int S, int H,
                             const float* cos, const float* sin, int split, const void* wqA, const void* wkA, const void* wqB, const void* wkB,
                             float eps, float scale, void* workspace, void* stream) {
  TD_CHECK_ARG(qkv && cos && sin && q_col >= 0 && k_col >= 0 && v_col >= 0 && (q_col | k_col | v_col) % 8 == 0, "td_attention_fp8_qk_rope: projection buffer, both tables, 16-byte aligned column offsets");
  TD_CHECK_ARG(S > 0 && H > 0 && (long long)(q_col > k_col ? (q_col > v_col ? q_col : v_col) : (k_col > v_col ? k_col : v_col)) + (long long)H * 128 <= ld,
               "td_attention_fp8_qk_rope: the q / k / v head blocks (H=%d x 128 columns from their offsets) do not fit a row of ld=%lld", H, (long long)ld);
  TdAttnParams p;
  p.Q = (const bf16_t*)qkv + q_col; p.K = (const bf16_t*)qkv + k_col; p.V = (const bf16_t*)qkv + v_col; p.O = (bf16_t*)o;
  p.batch = 1; p.Sq = S; p.Skv = S; p.Hq = H; p.Hkv = H; p.head_dim = 128;
  p.ldq = (int)ld; p.ldkv = (int)ld; p.ldo = (int)ldo; p.scale = scale; p.f8_ws = workspace; p.variant = ((g_attn_variant & 1) ? 0x1000 : 0) | ((g_attn_variant & 2) ? 0x2000 : 0);
  p.rope_cos = cos; p.rope_sin = sin; p.rope_split = split; p.rope_eps = eps;
  p.rope_wqA = (const bf16_t*)wqA; p.rope_wkA = (const bf16_t*)wkA; p.rope_wqB = (const bf16_t*)wqB; p.rope_wkB = (const bf16_t*)wkB;
  // q is rounded to bf16 as td_qk_norm_rope_bf16 leaves it and scaled in the pack pass, as td_attention_fp8 does (the FLUX engine folds the
  // scale in front of that rounding instead: TdQkRopeParams::q_premul on both of its paths)
  return td_attn_fp8_launch(p, (hipStream_t)stream);
}

int td_attention_varlen_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo,
                             const int* seg_starts, int n_seg, int max_len, int Hq, int Hkv, float scale, void* stream) {
  TD_CHECK_ARG(seg_starts && n_seg > 0 && max_len > 0, "td_attention_varlen: empty segment list");
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)o;
  p.batch = n_seg; p.Sq = max_len; p.Skv = max_len; p.Hq = Hq; p.Hkv = Hkv; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo;
  p.scale = scale; p.causal = 0; p.causal_offset = 0; p.variant = 1; p.seg_starts = seg_starts;
  return td_attn_launch(p, (hipStream_t)stream);
}

// td_attention_varlen_bf16 with a causal switch: TdAttnParams as the Qwen2-VL engine's packed prefill fills them (prefill_attn + seg_starts in
// csrc/qwen2_engine.hip: causal, causal_offset 0), so causal = 1 launches the engine's kernel instantiation.  Every refusal comes before the first HIP call.
int td_attention_segments_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo,
                               const int* seg_starts, int n_seg, int max_len, int Hq, int Hkv, float scale, int causal, void* stream) {
  TD_CHECK_ARG(seg_starts && n_seg > 0 && max_len > 0, "td_attention_segments: empty segment list");
  TD_CHECK_ARG(q && k && v && o, "td_attention_segments: null operand");
  TD_CHECK_ARG(causal == 0 || causal == 1, "td_attention_segments: causal=%d must be 0 or 1", causal);
  TD_CHECK_ARG(Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "td_attention_segments: Hq=%d not a positive multiple of Hkv=%d", Hq, Hkv);
  TD_CHECK_ARG(ldq >= (int64_t)Hq * 128 && ldkv >= (int64_t)Hkv * 128 && ldo >= (int64_t)Hq * 128 && ldq < (1ll << 31) && ldkv < (1ll << 31) && ldo < (1ll << 31),
               "td_attention_segments: a row stride (ldq=%lld ldkv=%lld ldo=%lld) is shorter than its heads or outside the 32-bit range", (long long)ldq, (long long)ldkv, (long long)ldo);
  TD_CHECK_ARG(ldq % 8 == 0 && ldkv % 8 == 0 && ldo % 4 == 0,
               "td_attention_segments: ldq=%lld and ldkv=%lld must be multiples of 8 elements (16 bytes), ldo=%lld of 4 (8 bytes)", (long long)ldq, (long long)ldkv, (long long)ldo);
  TD_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 == 0, "td_attention_segments: q, k, v and o must be 16-byte aligned");
  TD_CHECK_ARG((uintptr_t)seg_starts % 4 == 0, "td_attention_segments: seg_starts must be 4-byte aligned");
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)o;
  p.batch = n_seg; p.Sq = max_len; p.Skv = max_len; p.Hq = Hq; p.Hkv = Hkv; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo;
  p.scale = scale; p.causal = causal; p.causal_offset = 0; p.seg_starts = seg_starts;
  if (!causal) p.variant = 1;      // as td_attention_varlen_bf16 (the packed launch reads no variant; kept equal so that causal = 0 is that entry bit for bit)
  return td_attn_launch(p, (hipStream_t)stream);
}

// Packed causal query segments over key ranges of their own (context attention; TdAttnParams::kv_seg_row0 / kv_seg_lens as the Qwen2-VL engine's prefill
// behind cached prefixes fills them).  The refusals of td_attention_segments_bf16, before the first HIP call.
int td_attention_prefix_segments_bf16(const void* q, const void* k, const void* v, void* o, int64_t ldq, int64_t ldkv, int64_t ldo, const int* seg_starts,
                                      const int* kv_row0, const int* kv_lens, int n_seg, int max_q_len, int max_kv_len, int Hq, int Hkv, float scale, void* stream) {
  TD_CHECK_ARG(seg_starts && n_seg > 0 && max_q_len > 0, "td_attention_prefix_segments: empty segment list (n_seg=%d, max_q_len=%d)", n_seg, max_q_len);
  TD_CHECK_ARG(kv_row0 && kv_lens, "td_attention_prefix_segments: kv_row0 and kv_lens are both required (kv_row0 %s, kv_lens %s)", kv_row0 ? "set" : "null",
               kv_lens ? "set" : "null");
  TD_CHECK_ARG(max_kv_len >= max_q_len, "td_attention_prefix_segments: max_kv_len=%d is below max_q_len=%d (a segment has at least as many keys as queries)", max_kv_len, max_q_len);
  TD_CHECK_ARG(q && k && v && o, "td_attention_prefix_segments: null operand");
  TD_CHECK_ARG(Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "td_attention_prefix_segments: Hq=%d not a positive multiple of Hkv=%d", Hq, Hkv);
  TD_CHECK_ARG(ldq >= (int64_t)Hq * 128 && ldkv >= (int64_t)Hkv * 128 && ldo >= (int64_t)Hq * 128 && ldq < (1ll << 31) && ldkv < (1ll << 31) && ldo < (1ll << 31),
               "td_attention_prefix_segments: a row stride (ldq=%lld ldkv=%lld ldo=%lld) is shorter than its heads or outside the 32-bit range", (long long)ldq, (long long)ldkv, (long long)ldo);
  TD_CHECK_ARG(ldq % 8 == 0 && ldkv % 8 == 0 && ldo % 4 == 0,
               "td_attention_prefix_segments: ldq=%lld and ldkv=%lld must be multiples of 8 elements (16 bytes), ldo=%lld of 4 (8 bytes)", (long long)ldq, (long long)ldkv, (long long)ldo);
  TD_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 == 0, "td_attention_prefix_segments: q, k, v and o must be 16-byte aligned");
  TD_CHECK_ARG(((uintptr_t)seg_starts | (uintptr_t)kv_row0 | (uintptr_t)kv_lens) % 4 == 0, "td_attention_prefix_segments: seg_starts, kv_row0 and kv_lens must be 4-byte aligned");
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)o;
  p.batch = n_seg; p.Sq = max_q_len; p.Skv = max_kv_len; p.Hq = Hq; p.Hkv = Hkv; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo;
  p.scale = scale; p.causal = 1; p.seg_starts = seg_starts; p.kv_seg_row0 = kv_row0; p.kv_seg_lens = kv_lens;
  return td_attn_launch(p, (hipStream_t)stream);
}

int td_norm_rows_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int rows, int D, int rms, float eps,
                      const void* w, int split, const void* shiftA, const void* scaleA,
                      const void* shiftB, const void* scaleB, void* stream) {
  TdNormParams p;
  p.x = (const bf16_t*)x; p.ldx = (int)ldx; p.y = (bf16_t*)y; p.ldy = (int)ldy; p.rows = rows; p.D = D;
  p.rms = rms; p.eps = eps; p.w = (const bf16_t*)w; p.split = split;
  p.shiftA = (const bf16_t*)shiftA; p.scaleA = (const bf16_t*)scaleA;
  p.shiftB = (const bf16_t*)shiftB; p.scaleB = (const bf16_t*)scaleB;
  if (p.scaleA && !p.scaleB) { p.scaleB = p.scaleA; p.shiftB = p.shiftA; }
  return td_norm_rows_launch(p, (hipStream_t)stream);
}

int td_qk_norm_rope_bf16(void* qkv, int64_t ld, int rows, int Hq, int Hk, int q_col, int k_col,
                         const float* cos, const float* sin, int split, const void* wqA, const void* wkA,
                         const void* wqB, const void* wkB, float eps, int rotate_half, void* stream) {
  TdQkRopeParams p;
  p.qkv = (bf16_t*)qkv; p.ld = (int)ld; p.rows = rows; p.Hq = Hq; p.Hk = Hk; p.q_col = q_col; p.k_col = k_col;
  p.cos = cos; p.sin = sin; p.split = split;
  p.wqA = (const bf16_t*)wqA; p.wkA = (const bf16_t*)wkA; p.wqB = (const bf16_t*)wqB; p.wkB = (const bf16_t*)wkB;
  p.eps = eps; p.rotate_half = rotate_half;
  return td_qk_norm_rope_launch(p, (hipStream_t)stream);
}

// td_qk_norm_rope_bf16 with the factor the FLUX engine folds into q (TdQkRopeParams::q_premul), filled as the engine fills it
int td_qk_norm_rope_premul_bf16(void* qkv, int64_t ld, int rows, int Hq, int Hk, int q_col, int k_col,
                                const float* cos, const float* sin, int split, const void* wqA, const void* wkA,
                                const void* wqB, const void* wkB, float eps, int rotate_half, float q_premul, void* stream) {
  TdQkRopeParams p;
  p.qkv = (bf16_t*)qkv; p.ld = (int)ld; p.rows = rows; p.Hq = Hq; p.Hk = Hk; p.q_col = q_col; p.k_col = k_col;
  p.cos = cos; p.sin = sin; p.split = split;
  p.wqA = (const bf16_t*)wqA; p.wkA = (const bf16_t*)wkA; p.wqB = (const bf16_t*)wqB; p.wkB = (const bf16_t*)wkB;
  p.eps = eps; p.rotate_half = rotate_half;
  p.q_premul = q_premul;
  return td_qk_norm_rope_launch(p, (hipStream_t)stream);
}

int td_temb_combine_silu_bf16(const void* te, const void* ge, const void* pe, int n, int D, void* temb, void* silu_out, void* stream) {
  TD_CHECK_ARG(te && pe && silu_out, "td_temb_combine_silu: te, pe and silu_out are required (ge and temb may be null)");
  return td_temb_combine_silu_launch((const bf16_t*)te, (const bf16_t*)ge, (const bf16_t*)pe, n, D, (bf16_t*)temb, (bf16_t*)silu_out, (hipStream_t)stream);
}

int td_copy_cols_bf16(const void* src, int64_t lds, void* dst, int64_t ldd, int rows, int cols, void* stream) {
  TD_CHECK_ARG(lds >= 0 && lds < (1ll << 31) && ldd >= 0 && ldd < (1ll << 31), "td_copy_cols: lds=%lld / ldd=%lld outside the 32-bit range", (long long)lds, (long long)ldd);
  return td_copy_cols_launch((const bf16_t*)src, (int)lds, (bf16_t*)dst, (int)ldd, rows, cols, (hipStream_t)stream);
}

int td_fill_normal_from_bf16(void* dst, int64_t n, uint64_t seed, float std, float mean, int64_t pair0, void* stream) {
  TD_CHECK_ARG(pair0 >= 0, "td_fill_normal_from: pair0=%lld must not be negative", (long long)pair0);
  return td_fill_normal_from_launch((bf16_t*)dst, (long long)n, (unsigned long long)seed, std, mean, (long long)pair0, (hipStream_t)stream);
}

int td_flux_rope_table(const float* ids, int S, const int* axes_dims3, double theta, float* cos, float* sin, void* stream) {
  return td_flux_rope_table_launch(ids, S, axes_dims3, theta, cos, sin, (hipStream_t)stream);
}
int td_timestep_sincos(const float* t, int n, void* out, void* stream) {
  return td_timestep_sincos_launch(t, n, (bf16_t*)out, (hipStream_t)stream);
}
int td_euler_step_bf16(void* x, const void* v, float dt, int64_t n, void* stream) {
  return td_euler_step_launch((bf16_t*)x, (const bf16_t*)v, dt, n, (hipStream_t)stream);
}
int td_flux_inpaint_step_bf16(void* x, const void* v, const void* image_latents, const void* noise, const void* mask, float dt,
                              float sigma_next, int64_t n, void* stream) {
  return td_flux_inpaint_step_launch((bf16_t*)x, (const bf16_t*)v, (const bf16_t*)image_latents, (const bf16_t*)noise, (const bf16_t*)mask, dt,
                                     sigma_next, n, (hipStream_t)stream);
}
int td_flux_residual_inject_bf16(void* h, int64_t ldh, const void* r, int64_t ldr, int rows, int D, float scale, void* stream) {
  TD_CHECK_ARG(ldh >= 0 && ldh < (1ll << 31) && ldr >= 0 && ldr < (1ll << 31), "td_flux_residual_inject: ldh=%lld / ldr=%lld outside the 32-bit range", (long long)ldh, (long long)ldr);
  return td_flux_residual_inject_launch((bf16_t*)h, (int)ldh, (const bf16_t*)r, (int)ldr, rows, D, scale, (hipStream_t)stream);
}

int td_flux_residual_inject_multi_bf16(void* h, int64_t ldh, const void* const* r, const int64_t* ldr, const float* scales, int n, int rows, int D,
                                       void* stream) {
  TD_CHECK_ARG(h && r && ldr && scales, "td_flux_residual_inject_multi: null argument");
  TD_CHECK_ARG(n >= 1 && n <= TD_MAX_CONTROLNETS, "td_flux_residual_inject_multi: n=%d outside 1 .. %d", n, TD_MAX_CONTROLNETS);
  TD_CHECK_ARG(ldh >= 0 && ldh < (1ll << 31), "td_flux_residual_inject_multi: ldh=%lld outside the 32-bit range", (long long)ldh);
  int ld[TD_MAX_CONTROLNETS];
  for (int k = 0; k < n; ++k) {
    TD_CHECK_ARG(ldr[k] >= 0 && ldr[k] < (1ll << 31), "td_flux_residual_inject_multi: ldr[%d]=%lld outside the 32-bit range", k, (long long)ldr[k]);
    ld[k] = (int)ldr[k];
  }
  return td_flux_residual_inject_multi_launch((bf16_t*)h, (int)ldh, (const bf16_t* const*)r, ld, scales, n, rows, D, (hipStream_t)stream);
}

int td_block_cache_head_bf16(const void* h1, int64_t ld1, const void* h0, int64_t ld0, const void* r_prev, int64_t ldp, void* r, int64_t ldr, int rows, int D,
                             double* sums, void* ws, void* stream) {
  for (int64_t ld : {ld1, ld0, ldp, ldr}) TD_CHECK_ARG(ld >= 0 && ld < (1ll << 31), "td_block_cache_head: leading dimension %lld outside the 32-bit range", (long long)ld);
  return td_block_cache_head_launch((const bf16_t*)h1, (int)ld1, (const bf16_t*)h0, (int)ld0, (const bf16_t*)r_prev, (int)ldp, (bf16_t*)r, (int)ldr, rows, D, sums,
                                    (double*)ws, (hipStream_t)stream);
}

int td_block_cache_tail_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int rows, int D, void* stream) {
  for (int64_t ld : {lda, ldb, ldo}) TD_CHECK_ARG(ld >= 0 && ld < (1ll << 31), "td_block_cache_tail: leading dimension %lld outside the 32-bit range", (long long)ld);
  return td_block_cache_tail_launch((const bf16_t*)a, (int)lda, (const bf16_t*)b, (int)ldb, (bf16_t*)out, (int)ldo, rows, D, (hipStream_t)stream);
}
int td_redux_compose_bf16(const void* text, int64_t text_bstride, int T, const void* image, int64_t image_bstride, int S, const float* scales, int B, int D,
                          void* out, int64_t ldo, void* stream) {
  return td_redux_compose_launch((const bf16_t*)text, (long long)text_bstride, T, (const bf16_t*)image, (long long)image_bstride, S, scales, B, D, (bf16_t*)out,
                                 (long long)ldo, (hipStream_t)stream);
}
int td_flux_cfg_step_bf16(void* x, const void* v_pos, const void* v_neg, float scale, float dt, int64_t n, void* stream) {
  return td_flux_cfg_step_launch((bf16_t*)x, (const bf16_t*)v_pos, (const bf16_t*)v_neg, scale, dt, n, (hipStream_t)stream);
}
int td_flux_inpaint_mask(const void* mask, int format, int H, int W, int C, void* packed_out, void* stream) {
  return td_flux_inpaint_mask_launch(mask, format, H, W, C, (bf16_t*)packed_out, (hipStream_t)stream);
}
int td_flux_pack_latents(const void* src, void* dst, int C, int H, int W, int unpack, float div, float add, void* stream) {
  return td_flux_pack_launch((const bf16_t*)src, (bf16_t*)dst, C, H, W, unpack, div, add, (hipStream_t)stream);
}
int td_cls_avgpool2_bf16(const void* x, void* y, int G, int C, void* stream) {
  return td_cls_avgpool2_launch((const bf16_t*)x, (bf16_t*)y, G, C, (hipStream_t)stream);
}

int td_aligner_mlp2x_bf16(const void* x, int64_t ldx, int M, int K, int hidden, const void* w0, const void* b0,
                          const void* w2, const void* b2, const void* norm_w, float eps, int fp32_norm,
                          void* workspace, void* y, int64_t ldy, void* stream) {
  TD_CHECK_ARG(x && w0 && w2 && norm_w && workspace && y, "td_aligner_mlp2x: null argument");
  bf16_t* t0 = (bf16_t*)workspace;
  bf16_t* t1 = t0 + (size_t)M * hidden;
  TdGemmParams g;
  g.A = (const bf16_t*)x; g.lda = (int)ldx; g.W = (const bf16_t*)w0; g.bias = (const bf16_t*)b0;
  g.C = t0; g.ldc = hidden; g.M = M; g.N = hidden; g.K = K; g.act = TD_ACT_GELU_ERF;
  int rc = td_gemm_launch(g, (hipStream_t)stream);
  if (rc) return rc;
  TdGemmParams g2;
  g2.A = t0; g2.lda = hidden; g2.W = (const bf16_t*)w2; g2.bias = (const bf16_t*)b2;
  g2.C = t1; g2.ldc = hidden; g2.M = M; g2.N = hidden; g2.K = hidden;
  rc = td_gemm_launch(g2, (hipStream_t)stream);
  if (rc) return rc;
  TdNormParams n;
  n.x = t1; n.ldx = hidden; n.y = (bf16_t*)y; n.ldy = (int)ldy; n.rows = M; n.D = hidden;
  n.rms = fp32_norm ? 2 : 1; n.eps = eps; n.w = (const bf16_t*)norm_w;
  return td_norm_rows_launch(n, (hipStream_t)stream);
}

int td_embed_gather_bf16(const int* ids, const void* table, void* out, int n, int D, int vocab, void* stream) {
  return td_embed_gather_launch(ids, (const bf16_t*)table, (bf16_t*)out, n, D, vocab, (hipStream_t)stream);
}
int td_silu_mul_bf16(const void* gate_up, void* out, int rows, int I, void* stream) {
  return td_silu_mul_launch((const bf16_t*)gate_up, (bf16_t*)out, rows, I, (hipStream_t)stream);
}
int td_mrope_table(const int* pos3n, int n, const int* sections3, float theta, int round_bf16, float* cos, float* sin, void* stream) {
  return td_mrope_table_launch(pos3n, n, sections3, theta, round_bf16, cos, sin, (hipStream_t)stream);
}

int td_conv3x3_pack_weight(const void* w_oihw, void* w_packed, int Cout, int Cin, int Cout_pad, int Cin_pad, void* stream) {
  return td_conv_pack_launch((const bf16_t*)w_oihw, (bf16_t*)w_packed, Cout, Cin, Cout_pad, Cin_pad, (hipStream_t)stream);
}
// the two launches at the ends of td_vae_decode, alone (the engine calls the launchers with its own buffers: the null checks live here)
int td_vae_latents_to_nhwc_bf16(const void* packed, void* out, int C, int h, int w, int Cpad, float scaling_factor, float shift_factor, void* stream) {
  TD_CHECK_ARG(packed && out, "td_vae_latents_to_nhwc_bf16: null argument");
  TD_CHECK_ARG(h > 0 && w > 0, "td_vae_latents_to_nhwc_bf16: h=%d, w=%d must be positive (and even)", h, w);
  return td_latents_to_nhwc_launch((const bf16_t*)packed, (bf16_t*)out, C, h, w, Cpad, scaling_factor, shift_factor, (hipStream_t)stream);
}
int td_vae_image_finalize(const void* x, int P, int Cpad, void* image_u8, void* image_chw, void* stream) {
  TD_CHECK_ARG(x, "td_vae_image_finalize: null input");
  TD_CHECK_ARG(image_u8 || image_chw, "td_vae_image_finalize: no output asked for (image_u8 and image_chw are both null)");
  return td_image_finalize_launch((const bf16_t*)x, P, Cpad, (unsigned char*)image_u8, (bf16_t*)image_chw, (hipStream_t)stream);
}
int td_groupnorm_nhwc_bf16(const void* x, void* y, int P, int C, int groups, float eps, const void* gamma,
                           const void* beta, int silu, float* workspace, void* stream) {
  return td_groupnorm_nhwc_launch((const bf16_t*)x, (bf16_t*)y, P, C, groups, eps, (const bf16_t*)gamma, (const bf16_t*)beta, silu, workspace, (hipStream_t)stream);
}
int td_groupnorm_workspace_floats(void) { return 1024 * 64 * 2 + 256; }
int td_softmax_rows_f32_bf16(const float* s, void* p, int rows, int cols, float scale, void* stream) {
  return td_softmax_rows_launch(s, (bf16_t*)p, rows, cols, cols, scale, (hipStream_t)stream);
}
int td_softmax_rows_strided_f32_bf16(const float* s, void* p, int rows, int cols, int ld, float scale, void* stream) {
  return td_softmax_rows_launch(s, (bf16_t*)p, rows, cols, ld, scale, (hipStream_t)stream);
}

int td_layernorm_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int rows, int D, int rms, float eps,
                      const void* w, const void* b, void* stream) {
  return td_norm_rows_generic_launch((const bf16_t*)x, (int)ldx, (bf16_t*)y, (int)ldy, rows, D, rms, eps, (const bf16_t*)w, (const bf16_t*)b, (hipStream_t)stream);
}
int td_add_rows_bf16(const void* a, const void* b, void* out, int rows, int D, int b_rows, void* stream) {
  return td_add_rows_launch((const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out, rows, D, b_rows, (hipStream_t)stream);
}
int td_glu_mul_bf16(const void* gate_up, void* out, int rows, int I, int act, void* stream) {
  return td_glu_mul_launch((const bf16_t*)gate_up, (bf16_t*)out, rows, I, act, (hipStream_t)stream);
}
int td_attention_bias_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo,
                           int Sq, int Skv, int Hq, int Hkv, float scale, int causal, const float* bias, void* stream) {
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)o;
  p.batch = 1; p.Sq = Sq; p.Skv = Skv; p.Hq = Hq; p.Hkv = Hkv; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo;
  p.scale = scale; p.causal = causal; p.causal_offset = Skv - Sq; p.bias = bias;
  return td_attn_launch(p, (hipStream_t)stream);
}

int td_rope_half_bf16(void* x, int64_t ldx, int S, int H, int head_stride, int hd, const float* cos_t, const float* sin_t, void* stream) {
  return td_rope_half_launch((bf16_t*)x, (int)ldx, S, H, head_stride, hd, cos_t, sin_t, (hipStream_t)stream);
}
int td_vision_rope_table(const int* pos, int S, int hd, float theta, float* cos_t, float* sin_t, void* stream) {
  return td_vision_rope_table_launch(pos, S, hd, theta, cos_t, sin_t, (hipStream_t)stream);
}
int td_qwen2_patchify_u8(const void* img_hwc, int H, int W, const float* lut, int patch, int merge, int temporal, void* out, int Kpad, void* stream) {
  return td_qwen2_patchify_u8_launch((const unsigned char*)img_hwc, H, W, lut, patch, merge, temporal, (bf16_t*)out, Kpad, (hipStream_t)stream);
}

int td_resize_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk, int* ksize) {
  return td_resize_coeffs_host(in_size, out_size, filter, bounds, kk, ksize);
}

int td_image_resize_u8(const void* src_hwc, int in_h, int in_w, int in_c, void* dst_hwc, int out_h, int out_w, int out_c, const int32_t* h_bounds, const int32_t* h_kk,
                       int h_ksize, const int32_t* v_bounds, const int32_t* v_kk, int v_ksize, void* tmp, void* stream) {
  return td_image_resize_u8_launch((const unsigned char*)src_hwc, in_h, in_w, in_c, (unsigned char*)dst_hwc, out_h, out_w, out_c, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                   v_ksize, (unsigned char*)tmp, (hipStream_t)stream);
}

int td_image_lut_chw_f32(const void* img_hwc, int H, int W, int C, const float* lut, float* out, void* stream) {
  return td_image_lut_chw_f32_launch((const unsigned char*)img_hwc, H, W, C, lut, out, (hipStream_t)stream);
}

int td_patchify_bf16(const void* pix, int src_f32, int C, int H, int W, int p, void* out, int Kpad, void* stream) {
  return td_patchify_launch(pix, src_f32, C, H, W, p, (bf16_t*)out, Kpad, (hipStream_t)stream);
}
int td_cast_pad_rows_bf16(const void* src, int src_f32, int rows, int K, void* out, int Kpad, void* stream) {
  return td_cast_pad_rows_launch(src, src_f32, rows, K, (bf16_t*)out, Kpad, (hipStream_t)stream);
}

int td_quant_rows_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int K, void* stream) {
  return td_quant_rows_fp8_launch((const bf16_t*)x, (int)ldx, (uint8_t*)q, (int)ldq, scale, rows, K, (hipStream_t)stream);
}
int td_linear_fp8(const void* xq, int64_t ldx, const float* x_scale, const void* wq, const float* w_scale, const void* bias,
                  void* y, int64_t ldy, int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr,
                  int tile_cfg, void* stream) {
  TdGemmParams p;
  p.fp8 = 1; p.A = (const bf16_t*)xq; p.lda = (int)ldx; p.a_scale = x_scale;
  p.W = (const bf16_t*)wq; p.w_scale = w_scale; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y; p.ldc = (int)ldy;
  p.gate = (const bf16_t*)gate; p.res = (const bf16_t*)res; p.ldr = (int)ldr;
  p.M = M; p.N = N; p.K = K; p.act = act; p.cfg = tile_cfg;
  return td_gemm_launch(p, (hipStream_t)stream);
}
int td_quant_rows_int8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int K, void* stream) {
  return td_quant_rows_fp8_launch((const bf16_t*)x, (int)ldx, (uint8_t*)q, (int)ldq, scale, rows, K, (hipStream_t)stream, 1);
}
int td_linear_int8(const void* xq, int64_t ldx, const float* x_scale, const void* wq, const float* w_scale, const void* bias,
                   void* y, int64_t ldy, int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr,
                   int tile_cfg, void* stream) {
  TdGemmParams p;
  p.i8 = 1; p.A = (const bf16_t*)xq; p.lda = (int)ldx; p.a_scale = x_scale;
  p.W = (const bf16_t*)wq; p.w_scale = w_scale; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y; p.ldc = (int)ldy;
  p.gate = (const bf16_t*)gate; p.res = (const bf16_t*)res; p.ldr = (int)ldr;
  p.M = M; p.N = N; p.K = K; p.act = act; p.cfg = tile_cfg;
  return td_gemm_launch(p, (hipStream_t)stream);
}
int td_norm_rows_quant_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* q_scale, int rows, int D, int rms, float eps,
                           const void* w, int split, const void* shiftA, const void* scaleA, const void* shiftB, const void* scaleB,
                           void* stream) {
  TdNormParams p;
  p.x = (const bf16_t*)x; p.ldx = (int)ldx; p.q = (uint8_t*)q; p.ldq = (int)ldq; p.q_scale = q_scale; p.rows = rows; p.D = D;
  p.rms = rms; p.eps = eps; p.w = (const bf16_t*)w; p.split = split;
  p.shiftA = (const bf16_t*)shiftA; p.scaleA = (const bf16_t*)scaleA;
  p.shiftB = (const bf16_t*)shiftB; p.scaleB = (const bf16_t*)scaleB;
  if (p.scaleA && !p.scaleB) { p.scaleB = p.scaleA; p.shiftB = p.shiftA; }
  TD_CHECK_ARG(q && q_scale, "td_norm_rows_quant_fp8: null output");
  return td_norm_rows_launch(p, (hipStream_t)stream);
}

// ---- int8 policy building blocks (td_abi_version() >= 7): the launch forms only the FLUX engine used to reach, one thin entry each.  Every entry
// checks its pointers, alignments and extents itself, before the launcher makes its first HIP call (several launchers ask for the device first).
namespace {
inline bool al(const void* p, unsigned a) { return ((uintptr_t)p) % a == 0; }
inline bool ld32(int64_t ld) { return ld >= 0 && ld < (1ll << 31); }
}  // namespace

int td_norm_rows_quant8(const void* x, int64_t ldx, void* q, int64_t ldq, float* q_scale, int rows, int D, int rms, float eps,
                        const void* w, int split, const void* shiftA, const void* scaleA, const void* shiftB, const void* scaleB,
                        int int8, const void* smoothA, const void* smoothB, const int* extA, const int* extB, int ext_n, void* stream) {
  TD_CHECK_ARG(x && q && q_scale, "td_norm_rows_quant8: x, q and q_scale are required");
  TD_CHECK_ARG(rows > 0 && D > 0 && D % 512 == 0 && D <= 4096, "td_norm_rows_quant8: rows=%d, D=%d (a multiple of 512, at most 4096)", rows, D);
  TD_CHECK_ARG(ld32(ldx) && ld32(ldq) && ldx % 8 == 0 && ldx >= D && ldq % 8 == 0, "td_norm_rows_quant8: ldx=%lld / ldq=%lld must be multiples of 8, ldx >= D",
               (long long)ldx, (long long)ldq);
  TD_CHECK_ARG(al(x, 16) && al(w, 16) && al(shiftA, 16) && al(scaleA, 16) && al(shiftB, 16) && al(scaleB, 16) && al(smoothA, 16) && al(smoothB, 16),
               "td_norm_rows_quant8: x, w, the modulation rows and the smoothing factors must be 16-byte aligned");
  TD_CHECK_ARG(al(q, 8) && al(q_scale, 4), "td_norm_rows_quant8: misaligned rows: q must be 8-byte aligned, q_scale 4-byte");
  TD_CHECK_ARG((scaleA == nullptr) == (shiftA == nullptr) && (scaleB == nullptr) == (shiftB == nullptr) && (scaleA || !scaleB),
               "td_norm_rows_quant8: shift and scale come together (B without A is not a form)");
  TD_CHECK_ARG(ext_n >= 0 && (extA == nullptr) == (extB == nullptr) && (extA != nullptr) == (ext_n > 0), "td_norm_rows_quant8: replicated channels need both tables and ext_n > 0 (ext_n=%d)", ext_n);
  if (ext_n > 0) {
    TD_CHECK_ARG(int8 != 0, "td_norm_rows_quant8: replicated channels (ext tables) exist for the int8 form only");
    TD_CHECK_ARG(ext_n % 2 == 0 && al(extA, 4) && al(extB, 4), "td_norm_rows_quant8: ext_n=%d must be even, the tables 4-byte aligned", ext_n);
  }
  TD_CHECK_ARG(ldq >= (int64_t)D + ext_n, "td_norm_rows_quant8: ldq=%lld is less than D + ext_n = %d bytes", (long long)ldq, D + ext_n);
  TdNormParams p;
  p.x = (const bf16_t*)x; p.ldx = (int)ldx; p.q = (uint8_t*)q; p.ldq = (int)ldq; p.q_scale = q_scale; p.q_int8 = int8 ? 1 : 0; p.rows = rows; p.D = D;
  p.rms = rms; p.eps = eps; p.w = (const bf16_t*)w; p.split = split;
  p.shiftA = (const bf16_t*)shiftA; p.scaleA = (const bf16_t*)scaleA;
  p.shiftB = (const bf16_t*)shiftB; p.scaleB = (const bf16_t*)scaleB;
  if (p.scaleA && !p.scaleB) { p.scaleB = p.scaleA; p.shiftB = p.shiftA; }
  p.smoothA = (const bf16_t*)smoothA; p.smoothB = (const bf16_t*)smoothB;
  p.extA = extA; p.extB = extB; p.ext_n = ext_n;
  return td_norm_rows_launch(p, (hipStream_t)stream);
}

int td_quant_rows8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int K, int int8, const float* col_mul, uint32_t* amax_out, void* stream) {
  TD_CHECK_ARG(x && q && scale, "td_quant_rows8: x, q and scale are required");
  TD_CHECK_ARG(rows > 0 && K > 0 && K % 8 == 0, "td_quant_rows8: rows=%d, K=%d (a multiple of 8)", rows, K);
  TD_CHECK_ARG(ld32(ldx) && ld32(ldq) && ldx % 8 == 0 && ldq % 8 == 0 && ldx >= K && ldq >= K, "td_quant_rows8: ldx=%lld / ldq=%lld must be multiples of 8 and at least K",
               (long long)ldx, (long long)ldq);
  TD_CHECK_ARG(al(x, 16) && al(q, 8) && al(scale, 4) && al(amax_out, 4) && al(col_mul, 16), "td_quant_rows8: misaligned rows: x and col_mul 16-byte, q 8-byte, scale and amax_out 4-byte");
  return td_quant_rows_fp8_launch((const bf16_t*)x, (int)ldx, (uint8_t*)q, (int)ldq, scale, rows, K, (hipStream_t)stream, int8 ? 1 : 0, amax_out, col_mul);
}

int td_col_amax_bf16(const void* x, int64_t ldx, int rows, int K, uint32_t* amax, void* stream) {
  TD_CHECK_ARG(x && amax, "td_col_amax_bf16: x and amax are required");
  TD_CHECK_ARG(rows > 0 && K > 0 && K % 8 == 0 && ld32(ldx) && ldx % 8 == 0 && ldx >= K, "td_col_amax_bf16: rows=%d, K=%d, ldx=%lld (K and ldx multiples of 8, ldx >= K)", rows, K, (long long)ldx);
  TD_CHECK_ARG(al(x, 16) && al(amax, 4), "td_col_amax_bf16: misaligned rows: x must be 16-byte aligned, amax 4-byte");
  return td_col_amax_launch((const bf16_t*)x, (int)ldx, rows, K, amax, (hipStream_t)stream);
}

int td_smooth_factors(const uint32_t* amax_x, const uint32_t* amax_w, int n, float* s, float* inv, void* inv_bf16, void* stream) {
  TD_CHECK_ARG(amax_x && amax_w && s && inv && inv_bf16, "td_smooth_factors: both maxima and all three outputs are required");
  TD_CHECK_ARG(n > 0 && al(amax_x, 4) && al(amax_w, 4) && al(s, 4) && al(inv, 4) && al(inv_bf16, 2), "td_smooth_factors: n=%d must be positive, the arrays aligned to their element", n);
  return td_smooth_factors_launch(amax_x, amax_w, n, s, inv, (bf16_t*)inv_bf16, (hipStream_t)stream);
}

int td_q8_scales_from_amax(uint32_t* amax, float* scale, float* inv, int64_t n, float margin, void* stream) {
  TD_CHECK_ARG(amax && scale && inv, "td_q8_scales_from_amax: amax, scale and inv are required");
  TD_CHECK_ARG(n > 0 && al(amax, 4) && al(scale, 4) && al(inv, 4), "td_q8_scales_from_amax: n=%lld must be positive, the arrays 4-byte aligned", (long long)n);
  TD_CHECK_ARG(margin >= 1.0f, "td_q8_scales_from_amax: margin=%g below 1 would clip values the last step has seen", (double)margin);      // (false for NaN too)
  return td_q8_scales_from_amax_launch(amax, scale, inv, (long long)n, margin, (hipStream_t)stream);
}

int td_ext_cols_int8(void* q, int64_t ld, int rows, int K, const int* ext, int ext_n, void* stream) {
  TD_CHECK_ARG(q && ext && al(ext, 4), "td_ext_cols_int8: q and a 4-byte aligned ext table are required");
  TD_CHECK_ARG(rows > 0 && K > 0 && ext_n > 0 && ld32(ld) && ld >= (int64_t)K + ext_n, "td_ext_cols_int8: rows=%d, K=%d, ext_n=%d, ld=%lld (ld >= K + ext_n)", rows, K, ext_n, (long long)ld);
  return td_ext_cols_launch((uint8_t*)q, (int)ld, rows, K, ext, ext_n, (hipStream_t)stream);
}

namespace {
// what the three int8-output Linear entries share: one problem's operands and its int8 output of n_q8 columns
int q8_linear_check(const char* me, const TdLinearQ8Problem& a, int64_t ldx, int64_t ldq8, int N, int K, int n_q8, int act, int tile_cfg) {
  TD_CHECK_ARG(a.xq && a.x_scale && a.wq && a.w_scale, "%s: the int8 operands and their scales are required", me);
  TD_CHECK_ARG(a.q8, "%s: the int8 output q8 is required", me);
  TD_CHECK_ARG(a.q8_inv && a.q8_amax, "%s: the int8 output needs its per-row inverse scales (q8_inv) and its maxima accumulators (q8_amax)", me);
  TD_CHECK_ARG(a.M > 0 && N > 0 && K > 0 && K % 128 == 0, "%s: M=%d, N=%d, K=%d (K a multiple of 128)", me, a.M, N, K);
  TD_CHECK_ARG(n_q8 > 0 && n_q8 % 16 == 0 && N % 16 == 0, "%s: the int8 output is written 16 columns at a time: N=%d and its %d int8 columns must be multiples of 16", me, N, n_q8);
  TD_CHECK_ARG(ld32(ldx) && ld32(ldq8) && ldx % 16 == 0 && ldx >= K && ldq8 % 16 == 0 && ldq8 >= n_q8,
               "%s: ldx=%lld (>= K) and ldq8=%lld (>= the int8 columns) must be multiples of 16", me, (long long)ldx, (long long)ldq8);
  TD_CHECK_ARG(al(a.xq, 16) && al(a.wq, 16) && al(a.q8, 16) && al(a.bias, 16) && al(a.q8_smooth, 16) && al(a.x_scale, 4) && al(a.w_scale, 16) && al(a.q8_inv, 4) && al(a.q8_amax, 4),
               "%s: misaligned rows: xq, wq, q8, bias, q8_smooth and w_scale must be 16-byte aligned, the per-row arrays 4-byte", me);
  TD_CHECK_ARG(td_act_valid(act), "%s: unknown activation code %d", me, act);
  TD_CHECK_ARG(tile_cfg == -1 || tile_cfg == 0 || tile_cfg == 2, "%s: tile_cfg=%d: the int8 output exists on the 256-column tiles 0 (256x256) and 2 (32x256); -1 = automatic", me, tile_cfg);
  return 0;
}
void q8_linear_fill(TdGemmParams& p, const TdLinearQ8Problem& a, int64_t ldx, int64_t ldq8, int N, int K, int tile_cfg) {
  p.i8 = 1; p.A = (const bf16_t*)a.xq; p.lda = (int)ldx; p.a_scale = a.x_scale; p.W = (const bf16_t*)a.wq; p.w_scale = a.w_scale; p.bias = (const bf16_t*)a.bias;
  p.M = a.M; p.N = N; p.K = K; p.cfg = tile_cfg;
  p.q8 = (uint8_t*)a.q8; p.ldq8 = (int)ldq8; p.q8_inv = a.q8_inv; p.q8_amax = a.q8_amax; p.q8_smooth = (const bf16_t*)a.q8_smooth;
}
}  // namespace

int td_linear_int8_q8(const TdLinearQ8Problem* a, int64_t ldx, int64_t ldq8, int N, int K, int act, int tile_cfg, void* stream) {
  TD_CHECK_ARG(a, "td_linear_int8_q8: null problem");
  if (int rc = q8_linear_check("td_linear_int8_q8", *a, ldx, ldq8, N, K, N, act, tile_cfg)) return rc;
  TdGemmParams p;
  q8_linear_fill(p, *a, ldx, ldq8, N, K, tile_cfg);
  p.act = act; p.ldc = N;      // (no bf16 output in this form: C stays null and is never stored to)
  return td_gemm_launch(p, (hipStream_t)stream);
}

int td_linear_split_int8_q8(const TdLinearQ8Problem* a, int64_t ldx, int64_t ldq8, void* y0, int64_t ldy0, int act0, int act1, int N, int K, int n_split, int tile_cfg,
                            void* stream) {
  TD_CHECK_ARG(a, "td_linear_split_int8_q8: null problem");
  TD_CHECK_ARG(n_split > 0 && n_split < N && n_split % 256 == 0, "td_linear_split_int8_q8: n_split=%d must be a multiple of the 256-column tile inside (0, N=%d)", n_split, N);
  if (int rc = q8_linear_check("td_linear_split_int8_q8", *a, ldx, ldq8, N, K, N - n_split, act1, tile_cfg)) return rc;
  TD_CHECK_ARG(y0 && al(y0, 16) && ld32(ldy0) && ldy0 % 8 == 0 && ldy0 >= n_split, "td_linear_split_int8_q8: y0 must be 16-byte aligned with ldy0=%lld a multiple of 8, >= n_split", (long long)ldy0);
  TD_CHECK_ARG(td_act_valid(act0), "td_linear_split_int8_q8: unknown activation code %d", act0);
  TdGemmParams p;
  q8_linear_fill(p, *a, ldx, ldq8, N, K, tile_cfg);
  p.C = (bf16_t*)y0; p.ldc = (int)ldy0; p.act = act0; p.act2 = act1; p.n_split = n_split;
  // The kernel tells a split launch by a non-null C2, so one must be given; the int8 rows stand in and nothing is ever stored through it as bf16.
  // That rests on two things in gemm_bf16.hip: the Q8 epilogue returns after its int8 store, before the bf16 one, for every tile of the second
  // output; and plan_split_k() gives 1 part whenever i8 or q8 is set, so the split-K reduce kernel, which does store through C2, is never launched.
  p.C2 = (bf16_t*)a->q8; p.ldc2 = 0;
  return td_gemm_launch(p, (hipStream_t)stream);
}

int td_linear_grouped2_int8_q8(const TdLinearQ8Problem* a0, const TdLinearQ8Problem* a1, int64_t ldx, int64_t ldq8, int N, int K, int act, int tile_cfg, void* stream) {
  TD_CHECK_ARG(a0 && a1, "td_linear_grouped2_int8_q8: two problems are required");
  if (int rc = q8_linear_check("td_linear_grouped2_int8_q8 (problem 0)", *a0, ldx, ldq8, N, K, N, act, tile_cfg)) return rc;
  if (int rc = q8_linear_check("td_linear_grouped2_int8_q8 (problem 1)", *a1, ldx, ldq8, N, K, N, act, tile_cfg)) return rc;
  TdGemmParams p;
  q8_linear_fill(p, *a0, ldx, ldq8, N, K, tile_cfg);
  p.act = act; p.ldc = N;
  p.g_A = (const bf16_t*)a1->xq; p.g_a_scale = a1->x_scale; p.g_W = (const bf16_t*)a1->wq; p.g_w_scale = a1->w_scale; p.g_bias = (const bf16_t*)a1->bias; p.g_M = a1->M;
  p.g_q8 = (uint8_t*)a1->q8; p.g_q8_inv = a1->q8_inv; p.g_q8_amax = a1->q8_amax; p.g_q8_smooth = (const bf16_t*)a1->q8_smooth;
  // (no bf16 output in either problem: C and g_C stay null, which the launcher accepts of a q8 launch)
  return td_gemm_launch(p, (hipStream_t)stream);
}

namespace {
int attn_q8_check(const char* me, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* q8, int64_t ldq8, const float* q8_inv,
                  const uint32_t* q8_amax, int Sq, int Skv, int H) {
  TD_CHECK_ARG(q && k && v, "%s: q, k and v are required", me);
  TD_CHECK_ARG(q8, "%s: the int8 output q8 is required", me);
  TD_CHECK_ARG(q8_inv && q8_amax, "%s: the int8 output needs its per-row inverse scales (q8_inv) and its maxima accumulators (q8_amax)", me);
  TD_CHECK_ARG(Sq > 0 && Skv > 0 && H > 0 && H <= 65535, "%s: Sq=%d, Skv=%d, H=%d", me, Sq, Skv, H);
  TD_CHECK_ARG(ld32(ldq) && ld32(ldkv) && ld32(ldq8) && ldq % 8 == 0 && ldkv % 8 == 0 && ldq8 % 8 == 0 && ldq >= (int64_t)H * 128 && ldkv >= (int64_t)H * 128 && ldq8 >= (int64_t)H * 128,
               "%s: ldq=%lld, ldkv=%lld, ldq8=%lld must be multiples of 8 and at least H x 128", me, (long long)ldq, (long long)ldkv, (long long)ldq8);
  TD_CHECK_ARG(al(q, 16) && al(k, 16) && al(v, 16) && al(q8, 8) && al(q8_inv, 4) && al(q8_amax, 4), "%s: misaligned rows: q, k, v must be 16-byte aligned, q8 8-byte, the per-row arrays 4-byte", me);
  return 0;
}
}  // namespace

int td_attention_q8(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* q8, int64_t ldq8, const float* q8_inv, uint32_t* q8_amax,
                    int Sq, int Skv, int H, float scale, int causal, const float* bias, int q_prescaled, float score_bound, void* stream) {
  TD_CHECK_ARG(!causal && !bias, "td_attention_q8: the int8 output form exists for the joint attention only (no causal mask, no score bias)");
  if (int rc = attn_q8_check("td_attention_q8", q, ldq, k, v, ldkv, q8, ldq8, q8_inv, q8_amax, Sq, Skv, H)) return rc;
  TD_CHECK_ARG(score_bound >= 0.f && score_bound <= 48.f && (score_bound == 0.f || q_prescaled), "td_attention_q8: a score bound goes with pre-scaled q and lies in (0, 48] octaves (0 = none)");
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v;
  p.batch = 1; p.Sq = Sq; p.Skv = Skv; p.Hq = H; p.Hkv = H; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldq8; p.scale = q_prescaled ? 1.0f : scale; p.variant = g_attn_variant & 0xff;
  p.q_prescaled = q_prescaled ? 1 : 0; p.score_bound = score_bound;
  p.q8 = (uint8_t*)q8; p.ldq8 = (int)ldq8; p.q8_inv = q8_inv; p.q8_amax = q8_amax;
  return td_attn_launch(p, (hipStream_t)stream);
}

int td_attention_fp8_q8(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* q8, int64_t ldq8, const float* q8_inv, uint32_t* q8_amax,
                        int Sq, int Skv, int H, float scale, void* workspace, void* stream) {
  if (int rc = attn_q8_check("td_attention_fp8_q8", q, ldq, k, v, ldkv, q8, ldq8, q8_inv, q8_amax, Sq, Skv, H)) return rc;
  TD_CHECK_ARG(workspace && al(workspace, 16), "td_attention_fp8_q8: a 16-byte aligned workspace of td_attention_fp8_workspace_bytes(Sq, Skv, H) bytes is required");
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v;
  p.batch = 1; p.Sq = Sq; p.Skv = Skv; p.Hq = H; p.Hkv = H; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldq8; p.scale = scale; p.f8_ws = workspace;
  p.variant = ((g_attn_variant & 1) ? 0x1000 : 0) | ((g_attn_variant & 2) ? 0x2000 : 0);      // as td_attention_fp8 (without its timing probes)
  p.q8 = (uint8_t*)q8; p.ldq8 = (int)ldq8; p.q8_inv = q8_inv; p.q8_amax = q8_amax;
  return td_attn_fp8_launch(p, (hipStream_t)stream);
}

// ---- 8-bit weight stream (td_abi_version() >= 12): every entry checks its arguments itself, before the launcher makes its first HIP call
int td_quant_weight_rows_e4m3(const void* w, int64_t ldw, void* q, float* scale, void* w_hat, int N, int K, void* stream) {
  return td_quant_weight_rows_launch((const bf16_t*)w, (long long)ldw, (uint8_t*)q, scale, (bf16_t*)w_hat, N, K, (hipStream_t)stream);
}

namespace {
int w8_linear_check(const char* me, const void* x, int64_t ldx, const void* wq, const float* w_scale, const void* y, int64_t ldy, int M, int N, int K) {
  TD_CHECK_ARG(x && wq && w_scale && y, "%s: x, the 8-bit weights wq, their row scales w_scale and the output are required", me);
  TD_CHECK_ARG(M >= 1 && M <= 64, "%s: M=%d: the 8-bit weight stream takes 1 .. 64 rows (more rows read the bf16 weights through td_linear_bf16)", me, M);
  TD_CHECK_ARG(N > 0 && K > 0 && ld32(ldx) && ld32(ldy), "%s: N=%d, K=%d, ldx=%lld, ldy=%lld", me, N, K, (long long)ldx, (long long)ldy);
  return 0;
}
}  // namespace

int td_linear_w8_bf16(const void* x, int64_t ldx, const void* wq, const float* w_scale, const void* bias, void* y, int64_t ldy,
                      int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr, void* stream) {
  if (int rc = w8_linear_check("td_linear_w8_bf16", x, ldx, wq, w_scale, y, ldy, M, N, K)) return rc;
  TD_CHECK_ARG(ld32(ldr) && (!res || ldr >= N), "td_linear_w8_bf16: ldr=%lld must cover the N=%d columns of the residual", (long long)ldr, N);
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W8 = (const uint8_t*)wq; p.w8_scale = w_scale; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y; p.ldc = (int)ldy; p.gate = (const bf16_t*)gate; p.res = (const bf16_t*)res; p.ldr = (int)ldr;
  p.M = M; p.N = N; p.K = K; p.act = act;
  return td_gemv_launch(p, (hipStream_t)stream);
}

int td_linear_split_w8_bf16(const void* x, int64_t ldx, const void* wq, const float* w_scale, const void* bias, void* y0, int64_t ldy0, int act0,
                            void* y1, int64_t ldy1, int act1, int M, int N, int K, int n_split, void* stream) {
  if (int rc = w8_linear_check("td_linear_split_w8_bf16", x, ldx, wq, w_scale, y0, ldy0, M, N, K)) return rc;
  TD_CHECK_ARG(y1 && ld32(ldy1), "td_linear_split_w8_bf16: the second output y1 is required");
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W8 = (const uint8_t*)wq; p.w8_scale = w_scale; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y0; p.ldc = (int)ldy0; p.act = act0; p.C2 = (bf16_t*)y1; p.ldc2 = (int)ldy1; p.act2 = act1; p.n_split = n_split;
  p.M = M; p.N = N; p.K = K;
  return td_gemv_launch(p, (hipStream_t)stream);
}

int td_linear_glu_bf16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int M, int I, int K, void* stream) {
  TD_CHECK_ARG(x && w && y, "td_linear_glu_bf16: x, w and y are required");
  TD_CHECK_ARG(M >= 1 && M <= 64 && I > 0 && K > 0 && ld32(ldx) && ld32(ldy) && ldx >= K && ldy >= I, "td_linear_glu_bf16: M=%d (1 .. 64), I=%d, K=%d, ldx=%lld, ldy=%lld", M, I, K,
               (long long)ldx, (long long)ldy);
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W = (const bf16_t*)w; p.C = (bf16_t*)y; p.ldc = (int)ldy; p.M = M; p.N = I; p.K = K; p.glu_I = I;
  return td_gemv_launch(p, (hipStream_t)stream);
}

int td_linear_glu_w8_bf16(const void* x, int64_t ldx, const void* wq, const float* w_scale, void* y, int64_t ldy, int M, int I, int K, void* stream) {
  if (int rc = w8_linear_check("td_linear_glu_w8_bf16", x, ldx, wq, w_scale, y, ldy, M, I, K)) return rc;
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W8 = (const uint8_t*)wq; p.w8_scale = w_scale; p.C = (bf16_t*)y; p.ldc = (int)ldy; p.M = M; p.N = I; p.K = K; p.glu_I = I;
  return td_gemv_launch(p, (hipStream_t)stream);
}

// ---- 4-bit weight stream (td_abi_version() >= 20): as above, every refusal comes before the first HIP call
int td_quant_weight_rows_mxfp4(const void* w, int64_t ldw, void* packed, void* scales, void* w_hat, int N, int K, void* stream) {
  return td_quant_weight_rows_mxfp4_launch((const bf16_t*)w, (long long)ldw, (uint8_t*)packed, (uint8_t*)scales, (bf16_t*)w_hat, N, K, (hipStream_t)stream);
}

int td_dequant_rows_mxfp4(const void* packed, const void* scales, void* w_hat, int64_t ldw, int N, int K, void* stream) {
  return td_dequant_rows_mxfp4_launch((const uint8_t*)packed, (const uint8_t*)scales, (bf16_t*)w_hat, (long long)ldw, N, K, (hipStream_t)stream);
}

namespace {
int w4_linear_check(const char* me, const void* x, int64_t ldx, const void* packed, const void* scales, const void* y, int64_t ldy, int M, int N, int K) {
  TD_CHECK_ARG(x && packed && scales && y, "%s: x, the packed 4-bit weights, their block scales and the output are required", me);
  TD_CHECK_ARG(M >= 1 && M <= 64, "%s: M=%d: the 4-bit weight stream takes 1 .. 64 rows (more rows read the bf16 weights through td_linear_bf16)", me, M);
  TD_CHECK_ARG(N > 0 && K > 0 && ld32(ldx) && ld32(ldy), "%s: N=%d, K=%d, ldx=%lld, ldy=%lld", me, N, K, (long long)ldx, (long long)ldy);
  return 0;
}
}  // namespace

int td_linear_w4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* bias, void* y, int64_t ldy,
                      int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr, void* stream) {
  if (int rc = w4_linear_check("td_linear_w4_bf16", x, ldx, packed, scales, y, ldy, M, N, K)) return rc;
  TD_CHECK_ARG(ld32(ldr) && (!res || ldr >= N), "td_linear_w4_bf16: ldr=%lld must cover the N=%d columns of the residual", (long long)ldr, N);
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W4 = (const uint8_t*)packed; p.w4_scale = (const uint8_t*)scales; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y; p.ldc = (int)ldy; p.gate = (const bf16_t*)gate; p.res = (const bf16_t*)res; p.ldr = (int)ldr;
  p.M = M; p.N = N; p.K = K; p.act = act;
  return td_gemv_launch(p, (hipStream_t)stream);
}

int td_linear_split_w4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* bias, void* y0, int64_t ldy0, int act0,
                            void* y1, int64_t ldy1, int act1, int M, int N, int K, int n_split, void* stream) {
  if (int rc = w4_linear_check("td_linear_split_w4_bf16", x, ldx, packed, scales, y0, ldy0, M, N, K)) return rc;
  TD_CHECK_ARG(y1 && ld32(ldy1), "td_linear_split_w4_bf16: the second output y1 is required");
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W4 = (const uint8_t*)packed; p.w4_scale = (const uint8_t*)scales; p.bias = (const bf16_t*)bias;
  p.C = (bf16_t*)y0; p.ldc = (int)ldy0; p.act = act0; p.C2 = (bf16_t*)y1; p.ldc2 = (int)ldy1; p.act2 = act1; p.n_split = n_split;
  p.M = M; p.N = N; p.K = K;
  return td_gemv_launch(p, (hipStream_t)stream);
}

int td_linear_glu_w4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, void* y, int64_t ldy, int M, int I, int K, void* stream) {
  if (int rc = w4_linear_check("td_linear_glu_w4_bf16", x, ldx, packed, scales, y, ldy, M, I, K)) return rc;
  TdGemmParams p;
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.W4 = (const uint8_t*)packed; p.w4_scale = (const uint8_t*)scales; p.C = (bf16_t*)y; p.ldc = (int)ldy;
  p.M = M; p.N = I; p.K = K; p.glu_I = I;
  return td_gemv_launch(p, (hipStream_t)stream);
}

// ---- grouped int4 weight stream (td_abi_version() >= 22): as above, every refusal comes before the first HIP call
int td_repack_int4(int layout, const void* qweight, const void* qzeros, const void* scales_in, const void* g_idx, int N, int K, int G,
                   void* packed, void* scales, void* zeros, void* stream) {
  return td_repack_int4_launch(layout, (const int*)qweight, (const int*)qzeros, (const uint16_t*)scales_in, (const int*)g_idx, N, K, G, (uint8_t*)packed,
                               (uint16_t*)scales, (uint8_t*)zeros, (hipStream_t)stream);
}

int td_dequant_rows_int4(const void* packed, const void* scales, const void* zeros, int G, void* w_hat, int64_t ldw, int N, int K, void* stream) {
  return td_dequant_rows_int4_launch((const uint8_t*)packed, (const uint16_t*)scales, (const uint8_t*)zeros, G, (bf16_t*)w_hat, (long long)ldw, N, K, (hipStream_t)stream);
}

namespace {
// the checks the three int4 Linear entries share, and the weight operands into p
int i4_linear_args(const char* me, TdGemmParams& p, const void* x, int64_t ldx, const void* packed, const void* scales, const void* zeros, int G, const void* y,
                   int64_t ldy, int M, int N, int K) {
  TD_CHECK_ARG(x && packed && scales && zeros && y, "%s: x, the packed int4 weights, their group scales and zeros and the output are required", me);
  TD_CHECK_ARG(G == 32 || G == 64 || G == 128, "%s: G=%d: the group sizes served are 32, 64 and 128", me, G);
  TD_CHECK_ARG(M >= 1 && M <= 64, "%s: M=%d: the int4 weight stream takes 1 .. 64 rows (more rows read the bf16 weights through td_linear_bf16)", me, M);
  TD_CHECK_ARG(N > 0 && K > 0 && ld32(ldx) && ld32(ldy), "%s: N=%d, K=%d, ldx=%lld, ldy=%lld", me, N, K, (long long)ldx, (long long)ldy);
  p.A = (const bf16_t*)x; p.lda = (int)ldx; p.C = (bf16_t*)y; p.ldc = (int)ldy; p.M = M; p.N = N; p.K = K;
  p.I4 = (const uint8_t*)packed; p.i4_scale = (const uint16_t*)scales; p.i4_zero = (const uint8_t*)zeros; p.i4_gshift = G == 32 ? 5 : G == 64 ? 6 : 7;
  return 0;
}
}  // namespace

int td_linear_i4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* zeros, int G, const void* bias, void* y, int64_t ldy,
                      int M, int N, int K, int act, const void* gate, const void* res, int64_t ldr, void* stream) {
  TdGemmParams p;
  if (int rc = i4_linear_args("td_linear_i4_bf16", p, x, ldx, packed, scales, zeros, G, y, ldy, M, N, K)) return rc;
  TD_CHECK_ARG(ld32(ldr) && (!res || ldr >= N), "td_linear_i4_bf16: ldr=%lld must cover the N=%d columns of the residual", (long long)ldr, N);
  p.bias = (const bf16_t*)bias; p.gate = (const bf16_t*)gate; p.res = (const bf16_t*)res; p.ldr = (int)ldr; p.act = act;
  return td_gemv_launch(p, (hipStream_t)stream);
}

int td_linear_split_i4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* zeros, int G, const void* bias, void* y0,
                            int64_t ldy0, int act0, void* y1, int64_t ldy1, int act1, int M, int N, int K, int n_split, void* stream) {
  TdGemmParams p;
  if (int rc = i4_linear_args("td_linear_split_i4_bf16", p, x, ldx, packed, scales, zeros, G, y0, ldy0, M, N, K)) return rc;
  TD_CHECK_ARG(y1 && ld32(ldy1), "td_linear_split_i4_bf16: the second output y1 is required");
  p.bias = (const bf16_t*)bias; p.act = act0; p.C2 = (bf16_t*)y1; p.ldc2 = (int)ldy1; p.act2 = act1; p.n_split = n_split;
  return td_gemv_launch(p, (hipStream_t)stream);
}

int td_linear_glu_i4_bf16(const void* x, int64_t ldx, const void* packed, const void* scales, const void* zeros, int G, void* y, int64_t ldy, int M, int I,
                          int K, void* stream) {
  TdGemmParams p;
  if (int rc = i4_linear_args("td_linear_glu_i4_bf16", p, x, ldx, packed, scales, zeros, G, y, ldy, M, I, K)) return rc;
  p.glu_I = I;
  return td_gemv_launch(p, (hipStream_t)stream);
}

// ---- e4m3 KV cache (td_abi_version() >= 13): as above, every refusal comes before the first HIP call
int td_kv_quant_rows_e4m3(const void* kv, int64_t ld, void* q, int64_t ldq, float* scale, int64_t lds, void* kv_hat, int rows, int heads, const int* dst_rows, void* stream) {
  return td_kv_quant_rows_launch((const bf16_t*)kv, (long long)ld, (uint8_t*)q, (long long)ldq, scale, (long long)lds, (bf16_t*)kv_hat, rows, heads, dst_rows, (hipStream_t)stream);
}

int td_kv_dequant_rows_e4m3(const void* q, int64_t ldq, const float* scale, int64_t lds, void* out, int64_t ld, int rows, int heads, void* stream) {
  return td_kv_dequant_rows_launch((const uint8_t*)q, (long long)ldq, scale, (long long)lds, (bf16_t*)out, (long long)ld, rows, heads, (hipStream_t)stream);
}

int td_attention_decode_kv8(const void* q, int64_t ldq, int64_t q_bstride, const void* k8, const void* v8, int64_t ldkv, int64_t kv_bstride,
                            const float* k_scale, const float* v_scale, int64_t lds, int64_t s_bstride, void* o, int64_t ldo, int64_t o_bstride,
                            int batch, int Skv, const int* kv_lens, int Hq, int Hkv, float scale, void* stream) {
  TD_CHECK_ARG(q && k8 && v8 && k_scale && v_scale && o, "td_attention_decode_kv8: q, both byte planes (k8, v8), both scale planes (k_scale, v_scale) and o are required");
  TD_CHECK_ARG(batch > 0 && Skv > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "td_attention_decode_kv8: batch=%d, Skv=%d, Hq=%d, Hkv=%d (Hq a multiple of Hkv)", batch, Skv, Hq, Hkv);
  TD_CHECK_ARG(ld32(ldq) && ld32(ldkv) && ld32(ldo) && ld32(lds) && ldq % 8 == 0 && ldo % 8 == 0 && q_bstride % 8 == 0 && o_bstride % 8 == 0 && ldq >= (int64_t)Hq * 128 && ldo >= (int64_t)Hq * 128,
               "td_attention_decode_kv8: ldq=%lld, ldo=%lld must be multiples of 8 and at least Hq x 128", (long long)ldq, (long long)ldo);
  TD_CHECK_ARG(ldkv % 8 == 0 && kv_bstride % 8 == 0 && ldkv >= (int64_t)Hkv * 128, "td_attention_decode_kv8: ldkv=%lld, kv_bstride=%lld (bytes) must be multiples of 8, ldkv at least Hkv x 128",
               (long long)ldkv, (long long)kv_bstride);
  TD_CHECK_ARG(lds >= Hkv && s_bstride >= 0 && kv_bstride >= 0, "td_attention_decode_kv8: lds=%lld must cover the Hkv=%d scales of a row", (long long)lds, Hkv);
  TD_CHECK_ARG(al(q, 16) && al(o, 16) && al(k8, 8) && al(v8, 8) && al(k_scale, 4) && al(v_scale, 4) && al(kv_lens, 4),
               "td_attention_decode_kv8: misaligned operands: q and o must be 16-byte aligned, k8 and v8 8-byte, the scale planes and kv_lens 4-byte");
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.O = (bf16_t*)o; p.K8 = (const uint8_t*)k8; p.V8 = (const uint8_t*)v8; p.k_scale = k_scale; p.v_scale = v_scale;
  p.batch = batch; p.Sq = 1; p.Skv = Skv; p.Hq = Hq; p.Hkv = Hkv; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo; p.lds = (int)lds;
  p.q_bstride = q_bstride; p.kv_bstride = kv_bstride; p.o_bstride = o_bstride; p.s_bstride = s_bstride;
  p.scale = scale; p.causal = 1; p.causal_offset = Skv - 1; p.kv_lens = kv_lens;
  return td_attn_launch(p, (hipStream_t)stream);
}

// ---- speculative decoding (td_abi_version() >= 21): the launcher refuses before its first HIP call
int td_attention_verify_ex(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, int64_t kv_bstride, const void* k8, const void* v8,
                           const float* k_scale, const float* v_scale, int64_t lds, int64_t s_bstride, void* o, int64_t ldo, int n_seq,
                           const int32_t* seq_row0_dev, const int32_t* seq_rows_dev, const int32_t* seq_len0_dev, const int32_t* seq_slot_dev, int Hq, int Hkv,
                           float scale, int t_max, int max_len, void* stream) {
  TD_CHECK_ARG(max_len >= 0, "td_attention_verify: max_len=%d is negative (0 = unknown)", max_len);
  TD_CHECK_ARG(ld32(ldq) && ld32(ldkv) && ld32(ldo) && ld32(lds), "td_attention_verify: ldq=%lld, ldkv=%lld, ldo=%lld, lds=%lld must fit 32 bits", (long long)ldq,
               (long long)ldkv, (long long)ldo, (long long)lds);
  TdAttnParams p;
  p.Q = (const bf16_t*)q; p.O = (bf16_t*)o; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v;
  p.K8 = (const uint8_t*)k8; p.V8 = (const uint8_t*)v8; p.k_scale = k_scale; p.v_scale = v_scale;
  p.batch = n_seq; p.Sq = 1; p.Skv = max_len; p.Hq = Hq; p.Hkv = Hkv; p.head_dim = 128;
  p.ldq = (int)ldq; p.ldkv = (int)ldkv; p.ldo = (int)ldo; p.lds = (int)lds;
  p.kv_bstride = kv_bstride; p.s_bstride = s_bstride; p.scale = scale; p.causal = 1;
  p.vr_row0 = seq_row0_dev; p.vr_rows = seq_rows_dev; p.vr_len0 = seq_len0_dev; p.vr_slot = seq_slot_dev;
  return td_attn_verify_launch(p, t_max, (hipStream_t)stream);
}

int td_attention_verify(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, int64_t kv_bstride, const void* k8, const void* v8,
                        const float* k_scale, const float* v_scale, int64_t lds, int64_t s_bstride, void* o, int64_t ldo, int n_seq,
                        const int32_t* seq_row0_dev, const int32_t* seq_rows_dev, const int32_t* seq_len0_dev, const int32_t* seq_slot_dev, int Hq, int Hkv,
                        float scale, void* stream) {
  return td_attention_verify_ex(q, ldq, k, v, ldkv, kv_bstride, k8, v8, k_scale, v_scale, lds, s_bstride, o, ldo, n_seq, seq_row0_dev, seq_rows_dev, seq_len0_dev,
                                seq_slot_dev, Hq, Hkv, scale, TD_MAX_VERIFY_ROWS, 0, stream);
}

int td_sample_top_p_bf16(const void* logits, int64_t ld, int rows, int vocab, float temperature, float top_p,
                         uint64_t seed, uint64_t offset, int32_t* out_ids, void* stream) {
  TD_CHECK_ARG(logits && out_ids, "td_sample_top_p_bf16: null pointer");
  return td_sample_top_p_launch((const bf16_t*)logits, (long long)ld, rows, vocab, temperature, top_p, seed, offset, out_ids, (hipStream_t)stream);
}

}  // extern "C"
