// Internal launch interface between the kernel translation units and the C-ABI / engine.
// Not installed; the public surface is include/thinkdiff_hip.h.
#pragma once
#include "td_common.h"

enum TdAct { TD_ACT_NONE = 0, TD_ACT_GELU_TANH = 1, TD_ACT_GELU_ERF = 2, TD_ACT_SILU = 3, TD_ACT_QUICK_GELU = 4 };
// every launcher that takes an activation code refuses one outside this range (no route has a fallback for it)
inline bool td_act_valid(int act) { return act >= TD_ACT_NONE && act <= TD_ACT_QUICK_GELU; }

// (TdGemmArgs: what every GEMM / skinny-M kernel takes as its argument block; TdGemmParams below is what the launchers take)
struct TdGemmArgs {
  const bf16_t* A = nullptr;     // [M, lda]  activations, K-contiguous
  const bf16_t* W = nullptr;     // [N, K]    torch Linear weight layout
  const bf16_t* bias = nullptr;  // [N] or null
  bf16_t* C = nullptr;           // [M, ldc]
  const bf16_t* gate = nullptr;  // [N] or null : y *= gate[n]
  const bf16_t* res = nullptr;   // [M, ldr] or null : y += res[m,n]   (may alias C)
  bf16_t* C2 = nullptr;          // optional second output for columns >= n_split
  int M = 0, N = 0, K = 0;
  int lda = 0, ldc = 0, ldr = 0, ldc2 = 0;
  int n_split = 0;
  int act = TD_ACT_NONE, act2 = TD_ACT_NONE;
  // optional second problem of a grouped launch (same N, K, lda, ldc, ldr, act; own rows and weights):
  // the double-stream blocks run their text-token GEMM (M = 193) inside the image-token launch
  const bf16_t* g_A = nullptr; const bf16_t* g_W = nullptr; const bf16_t* g_bias = nullptr;
  const bf16_t* g_gate = nullptr; const bf16_t* g_res = nullptr; bf16_t* g_C = nullptr;
  int g_M = 0;
  int cfg = -1;                  // tile config override (-1: auto), see td_gemm_config_id
  // K split over workgroups (tile kernels, bf16 operands, plain / bias / residual / split-output epilogues): few output tiles and a long K -- the
  // KV-cached decode of 65-256 sequences, M <= 256 against N = hidden -- leave most CUs without a workgroup.  split_k = -1: the launcher decides
  // (parts so that tiles x parts covers the CUs, every part a whole number of k-tiles); > 1: that many parts; 0 / 1: none.  Part j contracts
  // K-range j of every tile into fp32 partial sums in sk_ws ([parts][M][N] floats; null: a pooled buffer of the (device, stream)), and a second launch
  // adds the parts in index order -- the result does not depend on the order the workgroups ran in -- and applies the epilogue with the tile
  // kernel's rounding points.  Forms the reduction does not cover (activation, gate, int8 / fp8, conv, grouped) are launched unsplit under -1.
  int split_k = 0;
  float* sk_ws = nullptr; long long sk_ws_bytes = 0;
  // split_k = -1 only, N % 512 == 0, N <= 4096, no second output: the reduction launch also RMS-normalises the finished row (Qwen2RMSNorm: the
  // arithmetic, summation order and rounding points of td_norm_rows_kernel's rms form on the bf16 row it has just written) into sk_norm_out
  // [M, sk_norm_ld] -- the norm launch that would follow the Linear (o_proj -> post_attention_layernorm, down_proj -> the next input_layernorm)
  // disappears.  The launch then always goes through the partial-sum buffer, with one part when a split does not pay.
  const bf16_t* sk_norm_w = nullptr; bf16_t* sk_norm_out = nullptr; int sk_norm_ld = 0; float sk_norm_eps = 1e-6f;
  int ldw = 0, k_parts = 1;      // filled by the launcher: row stride of W in elements (= the whole K), parts of a split launch (K = ONE part's extent)
  int out_f32 = 0;               // C is float* (ldc in floats): acc + bias stored unrounded, no act/gate/res
  // implicit-GEMM 3x3 convolution over an NHWC image (conv_H > 0): A = input [Hin*Win, Cin], W = [N, 9*Cin]
  // (k = tap*Cin + c, tap = ky*3+kx), M = conv_H*conv_W output pixels; conv_up = 1 fuses a nearest 2x upsample
  int conv_H = 0, conv_W = 0, conv_Cin = 0, conv_up = 0;
  // conv_s2 = 1: Downsample2D(padding=0)'s pad (0,1,0,1) + stride-2 3x3 conv instead; conv_H x conv_W is then the output extent
  // and the input is [2 conv_H * 2 conv_W, Cin] (a kernel form of its own: the stride-1 instantiations are untouched)
  int conv_s2 = 0;
  // fp8 operands (fp8 = 1): A and W hold OCP e4m3 bytes (lda, K in elements = bytes); y = acc * a_scale[m] * w_scale[n]
  // gated MLP in one pass (skinny-M kernels only, glu_I > 0): W = [gate rows | up rows] (2 * glu_I x K), N = glu_I outputs,
  // C[m, n] = bf16(bf16(silu(bf16(x.gate_n))) * bf16(x.up_n)) -- Linear, SiLU and the product each round, as the separate kernels do
  int glu_I = 0;
  int fp8 = 0;
  // 8-bit weight stream (skinny-M kernels only, M <= 64; W is then unused): W8 = OCP e4m3 bytes [N, K] (gated form: [2 glu_I, K]), w8_scale[n] = 2^e_n,
  // the format td_quant_weight_rows_launch writes.  The kernels convert with the row's scale inside the conversion, so the dot products / MFMAs see
  // the bf16 values q * 2^e exactly -- the operands the bf16 kernels see when W holds the dequantised weights; only the fp32 summation order may differ.
  const uint8_t* W8 = nullptr; const float* w8_scale = nullptr;
  // int8 operands (i8 = 1): A and W hold symmetric int8 (lda, K in elements = bytes), v_mfma_i32_16x16x64_i8, exact int32 accumulation;
  // y = float(acc) * a_scale[m] * w_scale[n] -- the same scale arrays and the same 2x-bf16 MFMA rate as the fp8 form
  int i8 = 0;
  // int8 OUTPUT of the activated result (int8 kernels, 256-wide tiles): q8[m, :] = clamp(rint(y * q8_inv[m]), +-127) with the caller's
  // per-row inverse scales, the maxima of |y| per row accumulated into q8_amax[m] (atomic max on float bits); with a split output
  // (C2) it applies to the second one, the first stays bf16.  g_* = the second problem of a grouped launch.  See the epilogue.
  uint8_t* q8 = nullptr; int ldq8 = 0; const float* q8_inv = nullptr; unsigned* q8_amax = nullptr;
  uint8_t* g_q8 = nullptr; const float* g_q8_inv = nullptr; unsigned* g_q8_amax = nullptr;
  // int8 OUTPUT only: per-column factors (bf16, indexed by the ABSOLUTE output column n of this launch; null = none) applied to the activated value
  // before its row maximum and its quantisation -- 1 / s of the int8 smoothing of the Linear that consumes this output
  const bf16_t* q8_smooth = nullptr; const bf16_t* g_q8_smooth = nullptr;
  const float* a_scale = nullptr; const float* w_scale = nullptr;        // [M], [N]
  const float* g_a_scale = nullptr; const float* g_w_scale = nullptr;    // second problem of a grouped launch
  int tiles_m = 0, tiles_m0 = 0, tiles_n = 0;  // filled by the launcher
  int ragged_rows = 64;                        // filled by the launcher: tiles with at most this many rows take the ragged loop (0 with TD_GEMM_NO_RAGGED: A/B)
  int tail_first_wg = 0;                       // filled by the launcher (tail-split launches): workgroups from here on take a sub-tile of the last tiles
  int no_tail = 0;                             // caller's hint: other kernels share the chip (several images in flight) -- an empty last round gets filled anyway, do not split it
  int probe = 0;                               // filled by the launcher from TD_GEMM_PROBE (timing experiments, results WRONG): 1 = no epilogue, 2 = no k-loop
  int drain_cap = 0;                           // 256x256 bf16 tile: at most this many persistent workgroups walk the tiles (0: one per CU); see td_gemm_bf16_drain_kernel
  // 4-bit weight stream (skinny-M kernels only, M <= 64; W and W8 are then unused): W4 = MXFP4 nibbles [N, K / 2] (gated form: [2 glu_I, K / 2]), element 2j in
  // the low nibble of byte j, w4_scale = e8m0 bytes [N, K / 32], the format td_quant_weight_rows_mxfp4_launch writes (csrc/mxfp4_pow2.h).  As with W8 the
  // kernels see the bf16 values q * 2^e exactly.  (At the end: the fields in front keep their places in the kernels' argument block.)
  const uint8_t* W4 = nullptr; const uint8_t* w4_scale = nullptr;
};

// ... plus the grouped int4 weight stream.  A part of its own: only the I4 forms of the skinny-M kernels take the whole struct, every other kernel takes the
// TdGemmArgs part, so its argument block -- and the code hipcc makes around it -- is what it was before this form existed.
struct TdGemmParams : TdGemmArgs {
  // grouped int4 weight stream (AWQ / GPTQ checkpoints; skinny-M kernels only, M <= 64; W, W8 and W4 are then unused): I4 = uint4 nibbles [N, K / 2] (gated
  // form: [2 glu_I, K / 2]), i4_scale = fp16 bits [N, K / G], i4_zero = zero points 0 .. 15 [N, K / G], i4_gshift = log2(G), G in {32, 64, 128}: the format
  // td_repack_int4_launch writes (csrc/int4_group.h).  The kernels see the bf16 values bf16_rne((q - z) s) exactly.
  const uint8_t* I4 = nullptr; const uint16_t* i4_scale = nullptr; const uint8_t* i4_zero = nullptr; int i4_gshift = 0;
};

int td_gemm_launch(const TdGemmParams& p, hipStream_t stream);
// weight-streaming form for M <= 8 (td_gemm_launch routes to it; csrc/gemv_bf16.hip)
int td_gemv_launch(const TdGemmParams& p, hipStream_t stream);
bool td_gemv_mfma_ok(const TdGemmParams& p);   // shapes the matrix-core weight stream takes for 16 < M <= 64
bool td_gemv_w8_ok(const TdGemmParams& p);     // shapes the 8-bit weight stream takes (p.W8 need not be set yet): what td_gemv_launch would accept with W8
// Weight-only e4m3 quantisation with one power-of-two scale per row (csrc/quant_weight.hip; the format: csrc/e4m3_pow2.h): q = the row's bytes,
// scale[n] = 2^e_n; w_hat (may be null, may alias w) = q 2^e_n as bf16, exactly
int td_quant_weight_rows_launch(const bf16_t* w, long long ldw, uint8_t* q, float* scale, bf16_t* w_hat, int N, int K, hipStream_t stream);
bool td_gemv_w4_ok(const TdGemmParams& p);     // shapes the 4-bit weight stream takes (p.W4 need not be set yet): what td_gemv_launch would accept with W4
// Weight-only MXFP4 quantisation, one e8m0 scale per 32 consecutive k of a row (csrc/quant_weight.hip; the format: csrc/mxfp4_pow2.h): packed [N, K / 2],
// scales [N, K / 32]; w_hat (may be null, may alias w) = q 2^e as bf16, exactly.  The second entry rebuilds w_hat from the bytes.
int td_quant_weight_rows_mxfp4_launch(const bf16_t* w, long long ldw, uint8_t* packed, uint8_t* scales, bf16_t* w_hat, int N, int K, hipStream_t stream);
int td_dequant_rows_mxfp4_launch(const uint8_t* packed, const uint8_t* scales, bf16_t* w_hat, long long ldw, int N, int K, hipStream_t stream);
bool td_gemv_i4_ok(const TdGemmParams& p);     // shapes the grouped int4 weight stream takes (p.I4 need not be set yet; p.i4_gshift must be)
// Grouped int4 (csrc/quant_weight.hip; the format: csrc/int4_group.h).  td_repack_int4_launch turns one checkpoint Linear -- layout 0: AutoAWQ "GEMM"
// (qweight int32 [K, N / 8], qzeros int32 [K / G, N / 8], scales fp16 [K / G, N]), 1: AutoGPTQ 4-bit (qweight int32 [K / 8, N], qzeros int32 [K / G, N / 8]
// stored as z - 1, scales fp16 [K / G, N]), 1 | 2: the same with checkpoint_format "gptq_v2" (zeros stored as they are) -- into packed [N, K / 2],
// scales fp16 [N, K / G], zeros uint8 [N, K / G] in one launch.  g_idx (may be null) is not read: only the trivial map k / G is served and the caller vouches
// for it.  td_dequant_rows_int4_launch yields w^ = bf16_rne((q - z) s) as bf16 [N, ldw].
int td_repack_int4_launch(int layout, const int* qweight, const int* qzeros, const uint16_t* scales_in, const int* g_idx, int N, int K, int G, uint8_t* packed,
                          uint16_t* scales, uint8_t* zeros, hipStream_t stream);
int td_dequant_rows_int4_launch(const uint8_t* packed, const uint16_t* scales, const uint8_t* zeros, int G, bf16_t* w_hat, long long ldw, int N, int K, hipStream_t stream);
// 0: 256x256 (td_gemm_bf16_nt_kernel<8,4>), 1: 256x64, 2: 32x256, 3: 288x192 (<9,3>)
int td_gemm_config_id(int M, int N, int K);
// The same choice under the caller's shared-chip hint (shared != 0; TdGemmParams::no_tail): the tile that costs the least CU time, per operand type
// (csrc/gemm_bf16.hip).  shared = 0 is td_gemm_config_id.  K in bf16 equivalents (operand bytes per row / 2).  What td_gemm_launch runs when cfg < 0.
enum { TD_OPERAND_BF16 = 0, TD_OPERAND_INT8 = 1, TD_OPERAND_E4M3 = 2 };
int td_gemm_plan(int M, int N, int K, int shared, int operand);

enum { TD_TRACE_GEMM_MAIN = 0, TD_TRACE_GEMM_OTHER = 1, TD_TRACE_ATTN = 2, TD_TRACE_NORM = 3, TD_TRACE_QKROPE = 4, TD_TRACE_GEMM_288 = 5, TD_TRACE_NCAT = 6 };

// q/k/v are read in place from projection outputs: token row s, head h at column h*128.
struct TdAttnParams {
  const bf16_t* Q = nullptr;  // [batch][Sq, ldq]
  const bf16_t* K = nullptr;  // [batch][Skv, ldkv]
  const bf16_t* V = nullptr;  // [batch][Skv, ldkv]
  bf16_t* O = nullptr;        // [batch][Sq, ldo]
  int batch = 1, Sq = 0, Skv = 0, Hq = 0, Hkv = 0, head_dim = 128;
  int ldq = 0, ldkv = 0, ldo = 0;
  long long q_bstride = 0, kv_bstride = 0, o_bstride = 0;  // elements
  float scale = 0.f;
  int causal = 0, causal_offset = 0;  // key visible iff key <= q + causal_offset
  int q_per_kv = 1;                   // filled by the launcher
  int variant = 0;                    // 0: shipped (lean stream), 1: first lockstep kernel (A/B only)
  // optional additive score bias (T5 relative position bias): fp32 [Hq, Sq, Skv]; scores = q.k*scale + bias
  const float* bias = nullptr;
  // optional per-batch cache length (device int[batch], causal kernel): sequence b attends keys [0, kv_lens[b]); Skv = the largest
  const int* kv_lens = nullptr;
  // decode kernel only (Sq = 1, kv_lens given): the step's rotary embedding and cache write happen INSIDE the attention launch.  Q then holds the RAW
  // q rows of the projection, dec_kv_new [batch, 2 Hkv 128] the raw new k | v rows, dec_cos / dec_sin fp32 [batch, 128] the tokens' M-RoPE table rows,
  // dec_row_off int[batch] the ROW index of each sequence's new cache row (x ldkv elements from K).  Every workgroup rotates its q heads and the new key
  // itself (rotate_half, every product rounded to bf16: td_decode_rope_scatter_kernel's arithmetic), uses the new key / value as the last of its
  // kv_lens[b] keys from registers, and the first workgroup of each kv head writes them to the cache -- nobody reads that row in this launch.
  const bf16_t* dec_kv_new = nullptr; const float* dec_cos = nullptr; const float* dec_sin = nullptr; const int* dec_row_off = nullptr;
  // decode kernel only: sequence b's cache is slot dec_slots[b] (K / V + dec_slots[b] kv_bstride) instead of slot b -- the sequences of a step need not
  // sit in the first slots, so a finished sequence frees its slot without anybody's cache rows being moved (continuous batching); q / o stay row b
  const int* dec_slots = nullptr;
  // td_attn_verify_launch only (device int[batch] each; batch = sequences): sequence b owns the q / o ROWS [vr_row0[b], vr_row0[b] + vr_rows[b]) (row stride
  // ldq / ldo), 1 <= vr_rows[b] <= TD_MAX_VERIFY_ROWS (clamped by the kernels), row j sees keys [0, vr_len0[b] + j) of cache slot vr_slot[b]
  const int* vr_row0 = nullptr; const int* vr_rows = nullptr; const int* vr_len0 = nullptr; const int* vr_slot = nullptr;
  int vr_tmax = 8;      // rows per sequence the launch is laid out for (filled by the launcher from its t_max): vr_rows[b] is clamped to 1..vr_tmax
  // decode kernel only: an e4m3 KV cache (K8 != null; K / V are then unused).  K8 / V8 [batch][Skv, ldkv] hold OCP e4m3 BYTES -- ldkv and kv_bstride count
  // bytes in this form -- and k_scale / v_scale [batch][Skv, lds] the power-of-two scale 2^e of every (row, kv head) (s_bstride floats between sequences):
  // the format td_kv_quant_rows_launch writes.  The kernel converts with the scale inside the conversion, so q.k and p.v see the bf16 values q 2^e exactly:
  // the arithmetic of the bf16 form on a cache that holds the dequantised rows.  With dec_kv_new, the new key and value are rounded through the format before
  // use and the first workgroup of each kv head writes their bytes and scales.
  const uint8_t* K8 = nullptr; const uint8_t* V8 = nullptr; const float* k_scale = nullptr; const float* v_scale = nullptr;
  int lds = 0; long long s_bstride = 0;
  // optional packed segments (device int[batch + 1], non-causal): segment b = rows [seg_starts[b], seg_starts[b+1]) of q/k/v/o; Sq = Skv = the longest
  const int* seg_starts = nullptr;
  // optional hand-off workspace of the persistent (stream-K) joint-attention kernel: td_attn_streamk_ws_bytes() bytes, zeroed
  // once by its owner, not shared by launches that may run concurrently (null: a per-(device, stream) one is created inside)
  void* sk_ws = nullptr;
  // q already carries scale * log2(e) (folded in where q was last rounded to bf16: TdQkRopeParams::q_premul), so scores arrive in
  // the exp2 domain and `scale` is not applied again; joint (non-causal, no bias / lengths / segments) attention only
  int q_prescaled = 0;
  // q_prescaled only: an upper bound of every score q'.k the caller can vouch for (FLUX: the QK-RMSNorm bounds |q'| and |k| by sqrt(128) x the
  // largest norm weight, so |q'.k| <= premul x 128 x max|w_q| x max|w_k| -- a per-block constant).  In (0, 48]: the kernels exponentiate the scores
  // as they are -- no reference point, no per-tile row maximum, no rescale (bf16 probabilities and fp32 sums do not care about magnitude:
  // exp2(+-48) and a sum of 2^13 of them are far inside the range); a score a few octaves above it is harmless.  0: the running-maximum form.
  float score_bound = 0.f;
  // int8 output instead of O (joint attention; the FLUX engine's history-scaled int8 mode): q8[b][row, head*128 + d] = clamp(rint(o * q8_inv[row]), +-127)
  // with the caller's per-row inverse scales, row maxima of |o| accumulated into q8_amax[row] (atomic max on float bits).  ldq8 in bytes.
  uint8_t* q8 = nullptr; int ldq8 = 0; const float* q8_inv = nullptr; unsigned* q8_amax = nullptr;
  // td_attn_fp8_launch only: td_attn_fp8_ws_bytes(Sq, Skv, Hq) bytes of scratch for the packed e4m3 operands
  void* f8_ws = nullptr;
  // td_attn_fp8_launch only: reference points carried from one denoise step to the next (ints, [Hq][Sq]).  ref_in (may be null): where each row's
  // softmax starts -- ceil(the row's largest score of the PREVIOUS step) - headroom, in log2 units -- instead of the first tile's maximum, so that
  // the reference hardly ever has to move (a move rescales O, the row sums and the scores: ~80 VALU instructions per wave); ref_out (may be null):
  // receives the same quantity of THIS launch (atomic max: both owners of a split item contribute); the launch's pack pass presets it.
  const int* ref_in = nullptr; int* ref_out = nullptr;
  // td_attn_fp8_launch only (rope_cos != null): Q / K are the RAW projection outputs and the pack pass applies the per-head
  // QK-RMSNorm + interleaved-pair rotary embedding of td_qk_norm_rope_kernel on its way (same arithmetic, same summation order and
  // the same bf16 rounding points: bit-identical to the two-pass form), so that pass and its HBM round trip disappear.  Needs
  // Sq == Skv (q and k rows are the same tokens); rows < rope_split take the A norm weights, the rest B (null: no norm).
  const float* rope_cos = nullptr; const float* rope_sin = nullptr;   // [Sq,128] fp32
  const bf16_t* rope_wqA = nullptr; const bf16_t* rope_wkA = nullptr; const bf16_t* rope_wqB = nullptr; const bf16_t* rope_wkB = nullptr;
  int rope_split = 0; float rope_eps = 1e-6f;
  float rope_q_premul = 1.0f;   // as TdQkRopeParams::q_premul (then q_prescaled = 1)
  // causal kernel, with seg_starts, both or neither (device int[batch] each): the packed query segments run over K / V ranges of their own -- prompts
  // continued behind cached prefixes.  Segment b's keys are rows [kv_seg_row0[b], kv_seg_row0[b] + kv_seg_lens[b]) of K / V (rows of ldkv), query row i of its
  // Sq_b rows sees keys 0 .. kv_seg_lens[b] - Sq_b + i.  Sq = the longest query segment (the grid), Skv = the longest key range (the descriptor check); the
  // kernel counts kv_seg_lens[b] < Sq_b as Sq_b.  (At the end: the fields in front keep their places in the kernels' argument block.)
  const int* kv_seg_row0 = nullptr; const int* kv_seg_lens = nullptr;
};
size_t td_attn_streamk_ws_bytes();
int td_attn_device_cus(int dev);
int td_attn_pooled_workspace(int dev, int ranges, hipStream_t stream, char** out);
// csrc/attention_fp8.hip: the joint attention with QK^T and P.V on the e4m3 MFMA (bf16 operands in, packed on the way)
size_t td_attn_fp8_ws_bytes(int Sq, int Skv, int H);
int td_attn_fp8_launch(const TdAttnParams& p, hipStream_t stream);

int td_attn_launch(const TdAttnParams& p, hipStream_t stream);
// Sq = 1 (KV-cached decode) form, csrc/attention_decode.hip; td_attn_launch routes to it
int td_attn_decode_launch(const TdAttnParams& p, hipStream_t stream);
// Multi-row decode attention (a speculative step's verify pass; csrc/attention_decode.hip): the vr_* layout of TdAttnParams, both cache forms.  t_max: the
// largest vr_rows[b] the caller vouches for (TD_MAX_VERIFY_ROWS when it cannot: the arrays are device memory); vr_rows[b] is clamped to 1..t_max, so a
// sequence never gets more rows than the grid was laid out for.  p.Skv: the longest visible length where the caller knows it (0 otherwise): routing only.
// td_attention_verify_set_form: 0 automatic, 1 one workgroup per row, 2 the multi-row kernel.
#ifndef TD_MAX_VERIFY_ROWS
#define TD_MAX_VERIFY_ROWS 8
#endif
int td_attn_verify_launch(const TdAttnParams& p, int t_max, hipStream_t stream);
// e4m3 KV-cache rows (csrc/attention_decode.hip; the layout of TdAttnParams::K8, the format of csrc/e4m3_pow2.h): every 128-wide head vector x of the
// `rows` bf16 rows kv [rows, ld] (`heads` vectors per row) becomes its 128 bytes at q[dst, h 128 ..] and its scale 2^e at scale[dst, h],
// dst = dst_rows[r] (device ints) or r.  kv_hat (may be null, may alias kv; row stride ld): x^ = q 2^e as bf16, exactly, at row r.  ldq in bytes, lds in floats.
int td_kv_quant_rows_launch(const bf16_t* kv, long long ld, uint8_t* q, long long ldq, float* scale, long long lds, bf16_t* kv_hat, int rows, int heads,
                            const int* dst_rows, hipStream_t stream);
// ... and back: out[r, h 128 + d] = q[r, h 128 + d] scale[r, h] as bf16 (exact)
int td_kv_dequant_rows_launch(const uint8_t* q, long long ldq, const float* scale, long long lds, bf16_t* out, long long ld, int rows, int heads, hipStream_t stream);
// ... row-mapped: out[r, :] = the dequantised row src_rows[r] (device ints) of q / scale -- the rows of several cache slots packed into one staging buffer in
// one launch (the packed prefill behind cached prefixes on an e4m3 cache)
int td_kv_dequant_rows_from_launch(const uint8_t* q, long long ldq, const float* scale, long long lds, bf16_t* out, long long ld, int rows, int heads,
                                   const int* src_rows, hipStream_t stream);
// csrc/flux_model.hip: td_fill_normal_bf16 whose element i draws what element 2 pair0 + i of a fill from pair 0 draws (a piece of a larger buffer).
// It exists for ONE caller: td_qwen2_init_random on a handle with the e4m3 cache, whose arena lacks the cache rows (td_qwen2::segs), so that the same seed
// gives the weights of a bf16-cache handle -- what tools/bench_qwen2_kv8.py's two-handle comparison needs.  Every other fill passes pair0 = 0.
int td_fill_normal_from_launch(bf16_t* dst, long long n, unsigned long long seed, float std, float mean, long long pair0, hipStream_t stream);

struct TdNormParams {
  const bf16_t* x = nullptr; int ldx = 0;
  bf16_t* y = nullptr; int ldy = 0;
  int rows = 0, D = 0;
  int rms = 0;        // 0: LayerNorm statistics (mean/var), 1: RMSNorm
  float eps = 1e-6f;
  const bf16_t* w = nullptr;  // optional affine weight [D]
  int split = 0;              // rows < split use set A, others set B
  const bf16_t* shiftA = nullptr; const bf16_t* scaleA = nullptr;
  const bf16_t* shiftB = nullptr; const bf16_t* scaleB = nullptr;
  // fp8 output (q != null): the row is written as OCP e4m3 q[row, :] = fp8(y / s), s = max|y| / 448 -> q_scale[row]; y unused
  uint8_t* q = nullptr; int ldq = 0; float* q_scale = nullptr;
  int q_int8 = 0;   // q holds symmetric int8 instead: q = rint(y / s), s = max|y| / 127
  // quantised output only: per-channel factors (bf16 [D], 1 / s of the int8 smoothing, powers of two) applied before the row maximum is taken;
  // A for rows < split, B for the others; null = none
  const bf16_t* smoothA = nullptr; const bf16_t* smoothB = nullptr;
  // ... and replicated channels (int8 only): q rows carry ext_n further bytes behind the D quantised ones, byte D + e = the quantised byte of
  // channel ext[e] (or 0 where ext[e] < 0).  A channel that runs r x above the rest is divided by r (smooth) and present r times -- the
  // contraction sums r x (x / r) w -- so its weight column keeps its magnitude and the row's step is set by the rest (outlier channel splitting).
  const int* extA = nullptr; const int* extB = nullptr; int ext_n = 0;
};
// weights of such a Linear: q[r, K + e] = q[r, ext[e]] (0 where ext[e] < 0) for every row of an int8 matrix with row stride ld >= K + ext_n
int td_ext_cols_launch(uint8_t* q, int ld, int rows, int K, const int* ext, int ext_n, hipStream_t stream);
// per-row dynamic fp8 quantisation of a bf16 matrix: q[r,:] = e4m3(x[r,:] / s_r), s_r = max|x[r,:]| / 448 (1 for a zero row)
// int8 = 1: symmetric int8 instead (q = rint(x / s_r), s_r = max|x[r,:]| / 127)
// col_mul (fp32 [K], may be null): per-column factors applied first (int8 smoothing: s on a weight's input channels, 1 / s on activations)
int td_quant_rows_fp8_launch(const bf16_t* x, int ldx, uint8_t* q, int ldq, float* scale, int rows, int K, hipStream_t stream, int int8 = 0, unsigned* amax_out = nullptr,
                             const float* col_mul = nullptr);
// int8 smoothing (csrc/elementwise.hip, bottom): column maxima of a bf16 matrix (atomic max into float bits), and the factors made from two of them
int td_col_amax_launch(const bf16_t* x, int ldx, int rows, int K, unsigned* amax, hipStream_t stream);
int td_smooth_factors_launch(const unsigned* ax, const unsigned* aw, int n, float* s, float* inv, bf16_t* inv16, hipStream_t stream);
// history-scaled int8 (csrc/elementwise.hip, bottom): turn the accumulated maxima into the next step's scales
int td_q8_scales_from_amax_launch(unsigned* amax, float* scale, float* inv, long long n, float margin, hipStream_t stream);
int td_norm_rows_launch(const TdNormParams& p, hipStream_t stream);

struct TdQkRopeParams {
  bf16_t* qkv = nullptr; int ld = 0;   // fused projection rows; modified in place
  int rows = 0, Hq = 0, Hk = 0;
  int q_col = 0, k_col = 0;            // first column of the q / k head blocks
  const float* cos = nullptr; const float* sin = nullptr;  // [rows,128] fp32
  int split = 0;
  const bf16_t* wqA = nullptr; const bf16_t* wkA = nullptr;  // rows < split (null: no norm)
  const bf16_t* wqB = nullptr; const bf16_t* wkB = nullptr;
  float eps = 1e-6f;
  int rotate_half = 0;  // 0: interleaved pairs (FLUX), 1: half-split fp32, 2: half-split with bf16 op rounding (Qwen2)
  // q (not k) is multiplied by this in fp32 before its one rounding to bf16: the attention scale * log2(e), so that the attention
  // kernel needs no per-score multiply (TdAttnParams::q_prescaled).  1 = the plain reference values.
  float q_premul = 1.0f;
};
int td_qk_norm_rope_launch(const TdQkRopeParams& p, hipStream_t stream);

int td_flux_rope_table_launch(const float* ids, int S, const int* axes, double theta, float* cosT, float* sinT, hipStream_t stream);
int td_timestep_sincos_launch(const float* t, int n, bf16_t* out, hipStream_t stream);
int td_temb_combine_silu_launch(const bf16_t* te, const bf16_t* ge, const bf16_t* pe, int n, int D, bf16_t* temb, bf16_t* silu_out, hipStream_t stream);
int td_euler_step_launch(bf16_t* x, const bf16_t* v, float dt, long long n, hipStream_t stream);
int td_flux_cfg_step_launch(bf16_t* x, const bf16_t* v_pos, const bf16_t* v_neg, float scale, float dt, long long n, hipStream_t stream);
int td_flux_residual_inject_launch(bf16_t* h, int ldh, const bf16_t* r, int ldr, int rows, int D, float scale, hipStream_t stream);
// n in 1 .. TD_MAX_CONTROLNETS samples folded in bf16, then added to h once (td_flux_residual_inject_multi_bf16 documents the rounding); r, ldr and
// scales are HOST arrays of n entries, passed on to the kernel by value
int td_flux_residual_inject_multi_launch(bf16_t* h, int ldh, const bf16_t* const* r, const int* ldr, const float* scales, int n, int rows, int D,
                                         hipStream_t stream);
// csrc/block_cache.hip: the first-block cache's residual + deterministic metric sums, and its tail difference (td_block_cache_*_bf16 document both)
int td_block_cache_head_launch(const bf16_t* h1, int ld1, const bf16_t* h0, int ld0, const bf16_t* r_prev, int ldp, bf16_t* r, int ldr, int rows, int D,
                               double* sums, double* ws, hipStream_t stream);
int td_block_cache_tail_launch(const bf16_t* a, int lda, const bf16_t* b, int ldb, bf16_t* out, int ldo, int rows, int D, hipStream_t stream);
// csrc/redux.hip: FLUX.1 Redux, B scaled [text | image] prompt streams summed into one (td_redux_compose_bf16 documents the rounding); validates its arguments
int td_redux_compose_launch(const bf16_t* text, long long text_bstride, int T, const bf16_t* image, long long image_bstride, int S, const float* scales,
                            int B, int D, bf16_t* out, long long ldo, hipStream_t stream);
// csrc/ip_attention.hip: FLUX IP-Adapter cross-attention (td_ip_attention_bf16 documents the arithmetic); validates its arguments
int td_ip_attention_launch(const bf16_t* q, int ldq, const bf16_t* k, const bf16_t* v, int ldkv, bf16_t* o, int ldo, int rows, int H, int n_keys,
                           const bf16_t* norm_w, float eps, float out_scale, int accumulate, hipStream_t stream);
int td_copy_cols_launch(const bf16_t* src, int lds, bf16_t* dst, int ldd, int rows, int cols, hipStream_t stream);
int td_flux_inpaint_step_launch(bf16_t* x, const bf16_t* v, const bf16_t* z, const bf16_t* noise, const bf16_t* mask, float dt,
                                float sigma_next, long long n, hipStream_t stream);
int td_flux_inpaint_mask_launch(const void* mask, int fmt, int H, int W, int C, bf16_t* out, hipStream_t stream);
int td_flux_pack_launch(const bf16_t* src, bf16_t* dst, int C, int H, int W, int unpack, float div, float add, hipStream_t stream);
int td_cls_avgpool2_launch(const bf16_t* x, bf16_t* y, int G, int C, hipStream_t stream);

int td_embed_gather_launch(const int* ids, const bf16_t* table, bf16_t* out, int n, int D, int vocab, hipStream_t stream);
int td_silu_mul_launch(const bf16_t* gu, bf16_t* out, int rows, int I, hipStream_t stream);
int td_mrope_table_launch(const int* pos, int n, const int* sections, float theta, int round_bf16, float* cosT, float* sinT, hipStream_t stream);

// VAE decoder kernels (vae_kernels.hip); groupnorm workspace: 1024*64*2 + 256 floats
int td_groupnorm_nhwc_launch(const bf16_t* x, bf16_t* y, int P, int C, int G, float eps, const bf16_t* gamma, const bf16_t* beta,
                             int silu, float* workspace, hipStream_t stream);
int td_softmax_rows_launch(const float* s, bf16_t* p, int rows, int cols, int ld, float scale, hipStream_t stream);   // ld: row stride of s and p (>= cols)
int td_conv_pack_launch(const bf16_t* w, bf16_t* out, int Cout, int Cin, int Cout_pad, int Cin_pad, hipStream_t stream);
int td_latents_to_nhwc_launch(const bf16_t* packed, bf16_t* out, int C, int h, int w, int Cpad, float div, float add, hipStream_t stream);
int td_image_finalize_launch(const bf16_t* x, int P, int Cpad, unsigned char* u8, bf16_t* chw, hipStream_t stream);
extern "C" int td_fill_normal_bf16(void* dst, int64_t n, uint64_t seed, float std, float mean, void* stream);

int td_norm_rows_generic_launch(const bf16_t* x, int ldx, bf16_t* y, int ldy, int rows, int D, int rms, float eps,
                                const bf16_t* w, const bf16_t* b, hipStream_t stream);
int td_add_rows_launch(const bf16_t* a, const bf16_t* b, bf16_t* out, int rows, int D, int b_rows, hipStream_t stream);
int td_glu_mul_launch(const bf16_t* gu, bf16_t* out, int rows, int I, int act, hipStream_t stream);
int td_rope_half_launch(bf16_t* x, int ldx, int S, int H, int head_stride, int hd, const float* cs, const float* sn, hipStream_t stream);
int td_vision_rope_table_launch(const int* pos, int S, int hd, float theta, float* cs, float* sn, hipStream_t stream);
int td_patchify_launch(const void* pix, int src_f32, int C, int H, int W, int p, bf16_t* out, int Kpad, hipStream_t stream);
int td_qwen2_patchify_u8_launch(const unsigned char* img, int H, int W, const float* lut, int p, int m, int T, bf16_t* out, int Kpad, hipStream_t stream);
int td_cast_pad_rows_launch(const void* src, int src_f32, int rows, int K, bf16_t* out, int Kpad, hipStream_t stream);

// csrc/image_resize.hip: PIL-exact separable resize of uint8 HWC images.  td_resize_coeffs_host fills one axis' table on the host (no HIP call, no
// allocation); the launch runs Pillow's horizontal then vertical pass (a pass whose size does not change is skipped) and validates its arguments.
int td_resize_coeffs_host(int in_size, int out_size, int filter, int* bounds, int* kk, int* ksize_out);
int td_image_resize_u8_launch(const unsigned char* src, int in_h, int in_w, int in_c, unsigned char* dst, int out_h, int out_w, int out_c, const int* h_bounds,
                              const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, unsigned char* tmp, hipStream_t stream);
// out fp32 [C, H, W] = lut[c][img[y, x, c]] for img uint8 [H, W, C]: an image processor's rescale + normalize as its own 256-entry table per channel
int td_image_lut_chw_f32_launch(const unsigned char* img, int H, int W, int C, const float* lut, float* out, hipStream_t stream);

// temperature / top-p sampling over bf16 logits rows (sampler.hip): one workgroup per row, token ids to out_ids[rows]
int td_sample_top_p_launch(const bf16_t* logits, long long ld, int rows, int vocab, float temperature, float top_p,
                           unsigned long long seed, unsigned long long offset, int* out_ids, hipStream_t stream);
