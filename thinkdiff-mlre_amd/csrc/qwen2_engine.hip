// Qwen2-VL text-decoder engine: hidden-state extraction at `model.norm` (the embedding ThinkDiff-LVLM feeds
// to its aligner) and KV-cached decoding, on the same GEMM / attention / row kernels as the FLUX engine.
//
// Replaces the vLLM fork's Qwen2-VL model runner behind `self.mllama.generate(..., return_hidden_states)`
// (reference thinkdiff/models/mllama_vllm_t5_embed_decoder_2.py:790-816,1083-1089 and
// thinkdiff/models/mllama_vllm_generate_1.py:382-413,586,614-615).  Per-layer math follows transformers
// `Qwen2VLDecoderLayer` (modeling_qwen2_vl.py:453-625), which SURVEY.md 8a row A7 identifies as identical:
//   h += o_proj(Attn(RMSNorm(h)));  h += down(SiLU(gate(x)) * up(x)), x = RMSNorm(h)
//   Attn: q/k/v Linear with bias, M-RoPE (rotate_half, 3 position streams merged by mrope_section),
//   causal GQA softmax(q k^T / sqrt(128)) v, o_proj without bias.
//
// Layout: one fused [q | k | v] projection per layer (dual-output GEMM epilogue: q to scratch, k | v to their own rows) and a KV
// cache of n_slots sequences x slot_len rows per layer.  Two layer loops:
//   prefill_pass -- many rows at once, in four forms that differ only in where a layer's k|v rows are written, what carries them
//     to the cache and what the attention reads (PrefillForm): one sequence at positions [pos0, pos0 + n) written straight into its
//     cache rows (td_qwen2_forward_slot), a right-padded batch (td_qwen2_prefill_batch_at), prompts back to back
//     (td_qwen2_prefill_packed_slots), prompts back to back behind cached prefixes (td_qwen2_prefill_packed_prefix_slots);
//   decode_step -- one new token for each of up to 256 sequences, with a launch list of its own (weight-stream or split-K Linears,
//     rotary embedding and cache write inside the attention launch), captured into a graph per batch size and replayed.
// Parameters are addressed by their Hugging Face names (model.layers.N.self_attn.q_proj.weight, ...).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "td_kernels.h"
#include "e4m3_pow2.h"
#include "qk_rope_math.h"
#include "../../include/thinkdiff_hip.h"

namespace {

struct QSlot { std::string name; bf16_t* ptr; int64_t count; };

// the quantised copy of one Linear weight (td_qwen2_quantize_weights): e4m3 bytes [N, K] and the fp32 row scales 2^e_n, or -- TD_QWEN2_WEIGHTS_MXFP4 --
// packed nibbles [N, K / 2] and the e8m0 block scale bytes [N, K / 32], or -- TD_QWEN2_WEIGHTS_INT4 (td_qwen2_load_param_int4) -- packed nibbles [N, K / 2],
// fp16 group scales [N, K / G] and zero points [N, K / G]; null on an unquantised handle (and for lm_head on an INT4 one)
struct W8Ref { uint8_t* q = nullptr; void* s = nullptr; uint8_t* z = nullptr; };

struct QLayer {
  W8Ref qkv_8, o_8, gu_8, down_8;
  bf16_t *qkv_w, *qkv_b;   // [(Hq + 2 Hkv) * 128, D]
  bf16_t* o_w;             // [D, Hq * 128]
  bf16_t* gu_w;            // [2 I, D] = gate_proj | up_proj
  bf16_t* down_w;          // [D, I]
  bf16_t *ln1_w, *ln2_w;   // [D]
  bf16_t* kv = nullptr;    // cache [max_tokens, 2 * Hkv * 128]; null on a handle with the e4m3 cache, which owns the two planes below instead
  uint8_t* kv8 = nullptr;  // e4m3 bytes [max_tokens, 2 * Hkv * 128], k heads then v heads
  float* kvs = nullptr;    // scales 2^e [max_tokens, 2 * Hkv]: column h = k head h, column Hkv + h = v head h
};

}  // namespace

struct td_qwen2 {
  TdQwen2Config cfg;
  int D = 0, I = 0, Hq = 0, Hkv = 0, max_tokens = 0;
  bf16_t* arena = nullptr;
  int64_t arena_elems = 0;
  std::vector<QSlot> slots;
  std::unordered_map<std::string, int> index;
  bf16_t *embed_w, *norm_w, *lm_w;
  std::vector<QLayer> layers;
  char* ws = nullptr;
  bf16_t *h, *xn, *q, *attn, *gu, *act;
  float *cosT, *sinT;
  // batched decode: the cache rows of every layer are split into n_slots sequences of slot_len rows
  int n_slots = 1, slot_len = 0, ws_rows = 0;
  bf16_t* kvtmp = nullptr;   // [ws_rows, 2 Hkv 128] k|v rows of a batched step before they are scattered to their sequences
  bf16_t* lastrows = nullptr; // [MAX_BATCH, D] last-token rows of a batched prefill (lm_head input)
  int* ibuf = nullptr;       // device ints: kv lengths, scatter offsets
  // Decode-step graphs.  A decode step is ~8 small launches per layer (230 for 28 layers) whose grids and arguments depend on the batch size
  // only -- sequence lengths and cache rows are device ints (ibuf), tokens / positions / outputs go through the fixed buffers below -- so the
  // step is captured once per (batch size, logits wanted) on the engine's own stream and replayed as ONE hipGraphLaunch on the caller's stream:
  // the GPU then runs the step's kernels back to back instead of waiting ~6 us for the host between them (the step was launch-bound: 1.5 ms
  // at one sequence of the 2B shape against 0.4 ms of weight streaming).  TD_QWEN2_NO_GRAPH: A/B and bisecting.
  std::unordered_map<int, hipGraphExec_t> step_graphs;
  std::unordered_map<int, int> step_calls;      // calls seen per key: the first runs eagerly (one-time function attributes are set outside a capture)
  hipStream_t capture_stream = nullptr;
  bool graphs_ok = true;
  bool fused_rope = true;                       // decode: rotary embedding + cache write inside the attention launch (td_qwen2_set_fused_rope)
  int *tok_buf = nullptr, *pos_buf = nullptr;   // [MAX_BATCH], [3, MAX_BATCH]: the step's token and position ids
  bf16_t* logits_buf = nullptr;                 // [MAX_BATCH, vocab]
  int* row_map = nullptr;                       // [ws_rows] packed prefill: cache row of every packed prompt row
  std::vector<int> row_map_host;                // ... its host image (kept alive across the asynchronous upload)
  // 8-bit / 4-bit weight stream (td_qwen2_quantize_weights): the e4m3 or MXFP4 copy (w_mode) of every Linear weight beside the bf16 arena, which then holds the dequantised values
  int w_mode = TD_QWEN2_WEIGHTS_BF16;
  bool w8_on = false;                           // launches of up to 64 rows read the 8-bit copy (td_qwen2_set_weight_stream)
  bool w8_stale = false;                        // parameters were loaded after quantising: every run is refused until td_qwen2_quantize_weights is called again
  char* w8_arena = nullptr;
  int64_t w8_bytes = 0;
  int w8_linears = 0;
  long long w8_launches = 0;                    // Linear launches enqueued (or captured) so far that read the 8-bit copy (td_qwen2_weight_stream_launches)
  W8Ref lm_8;
  // INT4: the group size of the copy (0: none yet) and which of the 7 x layers checkpoint Linears have int4 data (layer * 7 + q, k, v, o, gate, up, down)
  int i4_G = 0;
  std::vector<char> i4_have;
  int i4_loaded = 0;
  bool i4_route_all = false;                    // every row count the int4 forms take reads the copy, not only the measured-faster ones (td_qwen2_set_int4_routing)
  // e4m3 KV cache (td_qwen2_create_kv): fixed at creation, it sizes the allocation.  The parameter arena then lacks the cache rows; `segs` maps its pieces
  // (arena offset, offset in the bf16-mode layout, elements) so that td_qwen2_init_random draws the weights a bf16-mode handle draws from the same seed
  int kv_mode = TD_QWEN2_KV_BF16;
  char* kv8_arena = nullptr;
  struct Seg { int64_t off, voff, n; };
  std::vector<Seg> segs;
  int64_t voff_of(const bf16_t* p) const {
    const int64_t o = p - arena;
    for (const Seg& g : segs) if (o >= g.off && o < g.off + g.n) return g.voff + (o - g.off);
    return o;
  }
  // e4m3 cache, packed prefill behind cached prefixes (td_qwen2_prefill_packed_prefix_slots): the dequantised rows [0, prefix + len) of every sequence of a
  // pass, packed per segment, and the cache row of every staged row.  ws_rows rows each, allocated at the first such pass.
  bf16_t* kvstage = nullptr;
  int* stage_map = nullptr;
  float* sk_ws = nullptr;                       // partial sums of the decode step's split-K Linears (65-256 sequences): the engine's own buffer, so a captured step allocates nothing
  // Per-request LoRA (td_qwen2_lora_enable; csrc/lora_rows.hip): a pool of lora_max adapters x layers x 7 Linears of packed pairs, each place sized for
  // lora_max_rank; the row -> adapter array of a pass at a fixed device address (written before the pass, as ibuf is) and the kernels' workspace for ws_rows rows
  int lora_max = 0, lora_max_rank = 0;
  char* lora_arena = nullptr;
  int64_t lora_pool_bytes = 0;
  int64_t lora_place[7] = {0, 0, 0, 0, 0, 0, 0};   // byte offset of a Linear's place inside one (adapter, layer) block, and the block's size
  int64_t lora_block = 0;
  int* lora_rows = nullptr;                     // device int32 [ws_rows]
  char* lora_ws = nullptr;
  size_t lora_ws_bytes = 0;
  std::vector<char> lora_have;                  // [lora_max][layers][7]
  std::vector<int> lora_rank, lora_count;       // per adapter: its rank (one per adapter: rank_pattern is not served) and the pairs it holds
  std::vector<float> lora_scale;
  std::vector<int> slot_lora;                   // host map cache slot -> adapter (td_qwen2_lora_set_slot); slots past its end are -1
  std::vector<int> lora_rows_host;              // host image of lora_rows (kept alive across the asynchronous upload)
  long long lora_launches = 0;                  // low-rank launches enqueued (or captured) so far (td_qwen2_lora_info)
  int slot_adapter(int slot) const { return slot >= 0 && slot < (int)slot_lora.size() ? slot_lora[(size_t)slot] : -1; }
};

namespace {

void q_add(td_qwen2* f, const std::string& name, bf16_t* p, int64_t n) {
  f->index[name] = (int)f->slots.size();
  f->slots.push_back({name, p, n});
}

// Sequences per decode step (vLLM's max_num_seqs of the precompute job is 256: configs/qwen2_vl_embed_ccsbu.yaml:20).  Up to 64 the Linears of a step
// are weight streams (td_gemv_mfma_kernel: one pass over the weights for up to 64 rows); above, the step is a small-M GEMM problem and takes the tile
// kernels the prefill uses, with K split over workgroups where the output is narrow (td_gemm_launch's split_k form).
constexpr int MAX_BATCH = 256;
constexpr int STREAM_BATCH = 64;
constexpr int STREAM_ROWS_MAX = 64;            // rows the weight-stream kernels take (td_gemv_launch)
constexpr int64_t SK_WS_BYTES = 32ll << 20;

struct IntPack { int v[3 * MAX_BATCH]; };      // (3 KB of kernel arguments: lengths | cache rows | cache slots of a decode step)
__global__ void td_set_ints_kernel(int* dst, IntPack vals, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}

// row b*L + t of src -> cache row (b * slot_len + t): the k|v rows of a batched prefill go to their sequences' slots
__global__ void td_kv_rows_to_slots_kernel(const bf16_t* src, bf16_t* dst_base, int L, int slot_len, int W) {
  const int row = blockIdx.y;
  const int b = row / L, t = row - b * L;
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c < W) *(u32x4_t*)(dst_base + ((size_t)b * slot_len + t) * W + c) = *(const u32x4_t*)(src + (size_t)row * W + c);
}

// packed prefill: row r of src (prompts back to back) -> cache row dst_row[r] (its sequence's slot and position)
__global__ void td_kv_rows_to_rows_kernel(const bf16_t* src, bf16_t* dst_base, const int* dst_row, int W) {
  const int row = blockIdx.y;
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c < W) *(u32x4_t*)(dst_base + (size_t)dst_row[row] * W + c) = *(const u32x4_t*)(src + (size_t)row * W + c);
}
// dst[b, :] = src[seg_starts[b + 1] - 1, :]: the last row of every packed segment (lm_head input)
__global__ void td_gather_last_rows_kernel(const bf16_t* src, bf16_t* dst, const int* seg_starts, int D) {
  const int b = blockIdx.y;
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c < D) *(u32x4_t*)(dst + (size_t)b * D + c) = *(const u32x4_t*)(src + (size_t)(seg_starts[b + 1] - 1) * D + c);
}

// Decode step, one launch for: M-RoPE on the new q rows (in place), M-RoPE on the new k rows, k|v rows -> their sequences' cache
// rows.  Rotation = rotate_half with every op rounding to bf16 (qk_rope_half8_rbf: what td_qk_norm_rope_kernel does with rotate_half == 2).
// KV8: the rotated k and the v head vectors go through the e4m3 format (kv8_round_row: what the fused form does in the attention launch) and their
// bytes and scales are stored in cache8 / scales instead of the bf16 row.
template <bool KV8>
__global__ __launch_bounds__(256) void td_decode_rope_scatter_kernel(bf16_t* q, const bf16_t* kv, bf16_t* cache, uint8_t* cache8, float* scales, const int* row_off,
                                                                     const float* cosT, const float* sinT, int Hq, int Hkv) {
  const int b = blockIdx.x;
  const int l16 = threadIdx.x & 15, unit0 = threadIdx.x >> 4;
  const int QW = Hq * 128, KVW = 2 * Hkv * 128;
  float cs[8], sn[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { cs[i] = cosT[(size_t)b * 128 + l16 * 8 + i]; sn[i] = sinT[(size_t)b * 128 + l16 * 8 + i]; }
  bf16_t* dst = KV8 ? nullptr : cache + (size_t)row_off[b] * KVW;      // (row index of the sequence's new cache row)
  for (int u = unit0; u < Hq + 2 * Hkv; u += 16) {
    const bool is_q = u < Hq, is_v = u >= Hq + Hkv;
    const bf16_t* src = is_q ? q + (size_t)b * QW + u * 128 + l16 * 8 : kv + (size_t)b * KVW + (u - Hq) * 128 + l16 * 8;
    u32x4_t raw = *(const u32x4_t*)src;
    if (!is_v) {
      float x[8], other[8], y[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { x[2 * i] = bf_lo(raw[i]); x[2 * i + 1] = bf_hi(raw[i]); }
#pragma unroll
      for (int i = 0; i < 8; ++i) other[i] = __shfl_xor(x[i], 8, 16);
      qk_rope_half8_rbf(x, other, l16 < 8, cs, sn, y);
      raw = u32x4_t{pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]), pack_bf2(y[4], y[5]), pack_bf2(y[6], y[7])};
    }
    if constexpr (KV8) {
      if (is_q) {
        *(u32x4_t*)(q + (size_t)b * QW + u * 128 + l16 * 8) = raw;
      } else {      // (u is the same in all 16 lanes of a row, so the row is fully active here)
        float sc;
        const u32x2_t bytes = kv8_round_row(raw, sc);
        *(u32x2_t*)(cache8 + (size_t)row_off[b] * KVW + (u - Hq) * 128 + l16 * 8) = bytes;
        if (l16 == 0) scales[(size_t)row_off[b] * (2 * Hkv) + (u - Hq)] = sc;
      }
    } else {
      bf16_t* out = is_q ? q + (size_t)b * QW + u * 128 + l16 * 8 : dst + (u - Hq) * 128 + l16 * 8;
      *(u32x4_t*)out = raw;
    }
  }
}

// The launch arguments of one Linear, y[M, N] = x[M, K] W[N, K]^T (+ bias) (+ y itself with `residual`: the h += ... of both sub-blocks).
// Returned, not launched: the call sites with a second output or a K split decorate it first.
TdGemmParams linear(const bf16_t* x, int ldx, const bf16_t* W, const bf16_t* bias, bf16_t* y, int ldy, int M, int N, int K, bool residual = false) {
  TdGemmParams g;
  g.A = x; g.lda = ldx; g.W = W; g.bias = bias; g.C = y; g.ldc = ldy; g.M = M; g.N = N; g.K = K;
  if (residual) { g.res = y; g.ldr = ldy; }
  return g;
}

// INT4: the row counts at which the int4 forms measured FASTER than the bf16 kernels on W^ in both run orders (tools/bench_qwen2_int4.py with every
// bucket forced onto them, the int4_all column of profiles/qwen2_int4_bench.json): the unpack is VALU work the MXFP4 conversion instruction
// does not have, and at the other row counts it costs more than the bytes save.  Measured on the two decoder shapes at 1, 2, 4, 8, 16, 32 and 64 rows; the
// line between the shapes is drawn at the width that already separates them (hidden 3072), a row count between two buckets goes with the one above it.
// 7B shape: every bucket (x1.001 at 2 rows, x1.03 .. 1.31 elsewhere); 2B shape: 32 and 64 rows only (x1.07, x1.03; x0.81 .. 0.92 below).  Every other row
// count reads the bf16 arena.
bool int4_rows_routed(int M, int D) { return D >= 3072 ? M <= 64 : (M >= 17 && M <= 64); }

// Launches a Linear of the decoder.  With the weight stream on, a launch of up to 64 rows that would reach the skinny-M kernels anyway (no tile override,
// no K split) and has a shape their 8-bit (4-bit) forms take reads the quantised copy `w8` instead of the bf16 weight; everything else reads the bf16 arena,
// which holds the same (dequantised) values -- the model does not depend on the route.
int run_linear(td_qwen2* f, TdGemmParams g, const W8Ref& w8, hipStream_t s, bool allow8 = true) {
  if (allow8 && f->w8_on && w8.q && g.M <= STREAM_ROWS_MAX && g.cfg < 0 && g.split_k == 0) {
    if (f->w_mode == TD_QWEN2_WEIGHTS_INT4) {
      g.i4_gshift = f->i4_G == 32 ? 5 : f->i4_G == 64 ? 6 : 7;
      if ((f->i4_route_all || int4_rows_routed(g.M, f->D)) && td_gemv_i4_ok(g)) {
        g.I4 = w8.q; g.i4_scale = (const uint16_t*)w8.s; g.i4_zero = w8.z;
        ++f->w8_launches;
      }
    } else if (f->w_mode == TD_QWEN2_WEIGHTS_MXFP4 && td_gemv_w4_ok(g)) {
      g.W4 = w8.q; g.w4_scale = (const uint8_t*)w8.s;
      ++f->w8_launches;
    } else if (f->w_mode == TD_QWEN2_WEIGHTS_E4M3 && td_gemv_w8_ok(g)) {
      g.W8 = w8.q; g.w8_scale = (const float*)w8.s;
      ++f->w8_launches;
    }
  }
  return td_gemm_launch(g, s);
}

// logits[M, vocab] = lm_head(rows[M, hidden]), rows = model.norm outputs
int lm_head(td_qwen2* f, const bf16_t* rows, int M, void* logits, hipStream_t s, bool allow8 = true) {
  return run_linear(f, linear(rows, f->D, f->lm_w, nullptr, (bf16_t*)logits, f->cfg.vocab, M, f->cfg.vocab, f->D), f->lm_8, s, allow8);
}

// every entry that runs the model: a handle whose parameters changed after quantising is refused, never run half-quantised
#define TD_QWEN2_FRESH(f, fn)                                                                                                                                  \
  do {                                                                                                                                                         \
    TD_CHECK_ARG(!((f)->w8_stale && (f)->w_mode == TD_QWEN2_WEIGHTS_INT4),                                                                                     \
                 "%s: the handle holds int4 data for %d of its %d decoder Linears; give td_qwen2_load_param_int4 the rest first", fn, (f)->i4_loaded,         \
                 (int)(f)->i4_have.size());                                                                                                                    \
    TD_CHECK_ARG(!(f)->w8_stale, "%s: parameters were loaded after the weights were quantised; call td_qwen2_quantize_weights again first", fn);              \
  } while (0)

// two rows on one slot would write the same cache row: refused, not left to corrupt a sequence
int check_distinct_slots(const char* fn, const char* unit, const int* slots, int B) {
  int sorted[MAX_BATCH];
  std::copy(slots, slots + B, sorted);
  std::sort(sorted, sorted + B);
  const int* dup = std::adjacent_find(sorted, sorted + B);
  TD_CHECK_ARG(dup == sorted + B, "%s: cache slot %d is named by more than one %s", fn, *dup, unit);
  return TD_OK;
}

// k|v rows of one layer: in its cache from element `off` on, or (off < 0) in the engine's kvtmp
struct KvRows {
  long long off;
  bf16_t* of(const td_qwen2* f, const QLayer& l) const { return off < 0 ? f->kvtmp : l.kv + off; }
};
constexpr KvRows KV_TMP{-1};

// What tells the three prefills apart (everything else of prefill_pass is common to them).
struct PrefillForm {
  int n = 0;                   // rows of the pass
  KvRows kv_new = KV_TMP;      // where the q | k | v projection writes a layer's new k|v rows (RoPE rotates the k half there)
  // what carries them to the cache behind RoPE: nothing (they are cache rows), or one of
  const int* to_rows = nullptr;                // row r -> cache row to_rows[r] (device ints)
  long long to_slots = -1; int slots_L = 0;    // row b * slots_L + t -> row t of the b-th slot from cache element to_slots on
  TdAttnParams attn;           // the layer's attention, all but K / V, which are the k and the v half of `attn_kv`
  KvRows attn_kv = KV_TMP;
  // e4m3 cache: the new k | v rows always go to kvtmp, from row q8_tmp_row0 on; behind RoPE td_kv_quant_rows_launch writes their bytes and scales to cache row
  // to_rows[r], or (to_rows null) q8_cache_row0 + q8_tmp_row0 + r, and puts x^ back into kvtmp, which the attention reads (attn_kv = KV_TMP).  A continuation
  // (q8_tmp_row0 > 0) first dequantises cache rows [q8_cache_row0, q8_cache_row0 + q8_tmp_row0) into kvtmp rows [0, q8_tmp_row0): exact, x^ is a bf16 value.
  int q8_tmp_row0 = 0; long long q8_cache_row0 = 0;
  // e4m3 cache behind cached prefixes (q8_stage_n > 0; to_rows given): once the new rows are in the cache, cache row q8_stage_rows[r] (device ints) is
  // dequantised into row r of f->kvstage for r < q8_stage_n -- every sequence's rows [0, prefix + len), packed per segment -- and the attention reads kvstage
  const int* q8_stage_rows = nullptr; int q8_stage_n = 0;
  bool lora = false;           // some row names an adapter (f->lora_rows is written): the low-rank add follows each of the four Linears
};

// The low-rank add behind one fused Linear of layer `layer` (td_lora_rows_bf16): segments m0 .. m0 + n_segs - 1 of the 7 Linears (q, k, v, o, gate, up, down)
// on one input x [rows, K], segment i into y[i].  The rows' adapters are in f->lora_rows already.  Nothing is launched where no resident adapter holds a
// pair for one of the segments.
int lora_add(td_qwen2* f, int layer, int m0, int n_segs, const bf16_t* x, int ldx, int rows, int K, bf16_t* const* y, const int64_t* ldy, const int* widths,
             hipStream_t s) {
  const void* packed[TD_LORA_MAX_ADAPTERS * TD_LORA_ROWS_MAX_SEGS];
  bool any = false;
  for (int a = 0; a < f->lora_max; ++a)
    for (int i = 0; i < n_segs; ++i) {
      const bool have = f->lora_have[((size_t)a * f->layers.size() + layer) * 7 + m0 + i] != 0;
      packed[a * n_segs + i] = have ? f->lora_arena + ((size_t)a * f->layers.size() + layer) * f->lora_block + f->lora_place[m0 + i] : nullptr;
      any = any || have;
    }
  if (!any) return TD_OK;
  f->lora_launches += 2;      // shrink + expand
  return td_lora_rows_bf16(x, ldx, rows, K, f->lora_rows, f->lora_max, packed, f->lora_rank.data(), f->lora_scale.data(), n_segs, (void* const*)y, ldy, widths,
                           f->lora_ws, f->lora_ws_bytes, s);
}
int lora_add_qkv(td_qwen2* f, int layer, bf16_t* kv_new, int rows, hipStream_t s) {
  const int QW = f->Hq * 128, HW = f->Hkv * 128;
  bf16_t* y[3] = {f->q, kv_new, kv_new + HW};
  const int64_t ldy[3] = {QW, 2 * HW, 2 * HW};
  const int widths[3] = {QW, HW, HW};
  return lora_add(f, layer, 0, 3, f->xn, f->D, rows, f->D, y, ldy, widths, s);
}
int lora_add_o(td_qwen2* f, int layer, int rows, hipStream_t s) {
  bf16_t* y[1] = {f->h};
  const int64_t ldy[1] = {f->D};
  const int widths[1] = {f->D};
  return lora_add(f, layer, 3, 1, f->attn, f->Hq * 128, rows, f->Hq * 128, y, ldy, widths, s);
}
int lora_add_gu(td_qwen2* f, int layer, int rows, hipStream_t s) {
  bf16_t* y[2] = {f->gu, f->gu + f->I};
  const int64_t ldy[2] = {2 * f->I, 2 * f->I};
  const int widths[2] = {f->I, f->I};
  return lora_add(f, layer, 4, 2, f->xn, f->D, rows, f->D, y, ldy, widths, s);
}
int lora_add_down(td_qwen2* f, int layer, int rows, hipStream_t s) {
  bf16_t* y[1] = {f->h};
  const int64_t ldy[1] = {f->D};
  const int widths[1] = {f->D};
  return lora_add(f, layer, 6, 1, f->act, f->I, rows, f->I, y, ldy, widths, s);
}

// The rows' adapters of a pass -> f->lora_rows, from the host image the entry filled; false (nothing uploaded: the pass is the adapter-less one) where LoRA is
// off or no row names an adapter.  rc: the upload's status.
bool lora_upload_rows(td_qwen2* f, int n, hipStream_t s, int* rc) {
  *rc = TD_OK;
  if (f->lora_max == 0) return false;
  bool any = false;
  for (int r = 0; r < n; ++r) any = any || f->lora_rows_host[(size_t)r] >= 0;
  if (!any) return false;
  if (hipMemcpyAsync(f->lora_rows, f->lora_rows_host.data(), (size_t)n * 4, hipMemcpyHostToDevice, s) != hipSuccess) {
    td_set_error("td_qwen2: the upload of the row -> adapter array failed");
    *rc = TD_ERR_HIP;
  }
  return true;
}

// Runs form.n rows through the decoder: embed (or take inputs_embeds), M-RoPE table, every layer, model.norm -- left in f->xn and copied to
// hidden_out if given.  The caller has checked its arguments; which rows feed lm_head is its business too.
int prefill_pass(td_qwen2* f, const PrefillForm& form, const int* token_ids, const void* inputs_embeds, const int* position_ids, void* hidden_out, hipStream_t s) {
  const int D = f->D, I = f->I, Hq = f->Hq, Hkv = f->Hkv, n = form.n;
  const int QW = Hq * 128, KVW = 2 * Hkv * 128;

  if (inputs_embeds) TD_CHECK_HIP(hipMemcpyAsync(f->h, inputs_embeds, (size_t)n * D * 2, hipMemcpyDeviceToDevice, s));
  else TD_TRY(td_embed_gather_launch(token_ids, f->embed_w, f->h, n, D, f->cfg.vocab, s));
  // transformers casts the fp32 cos/sin tables to the model dtype before use
  TD_TRY(td_mrope_table_launch(position_ids, n, f->cfg.mrope_section, f->cfg.rope_theta, 1, f->cosT, f->sinT, s));

  TdNormParams np;
  np.x = f->h; np.ldx = D; np.y = f->xn; np.ldy = D; np.rows = n; np.D = D; np.rms = 1; np.eps = f->cfg.rms_eps;
  TdQkRopeParams rq;   // q heads in the q buffer
  rq.qkv = f->q; rq.ld = QW; rq.rows = n; rq.Hq = Hq; rq.Hk = 0; rq.q_col = 0; rq.k_col = 0;
  rq.cos = f->cosT; rq.sin = f->sinT; rq.rotate_half = 2;
  TdQkRopeParams rk = rq;  // k heads in the k|v rows just written
  rk.ld = KVW; rk.Hq = Hkv;
  TdAttnParams ap = form.attn;
  const bool kv8 = f->kv_mode == TD_QWEN2_KV_E4M3;

  for (int li = 0; li < (int)f->layers.size(); ++li) {
    const QLayer& l = f->layers[(size_t)li];
    bf16_t* kv_new = kv8 ? f->kvtmp + (size_t)form.q8_tmp_row0 * KVW : form.kv_new.of(f, l);
    if (kv8 && form.q8_tmp_row0 > 0)
      TD_TRY(td_kv_dequant_rows_launch(l.kv8 + (size_t)form.q8_cache_row0 * KVW, KVW, l.kvs + (size_t)form.q8_cache_row0 * 2 * Hkv, 2 * Hkv, f->kvtmp, KVW,
                                       form.q8_tmp_row0, 2 * Hkv, s));
    np.w = l.ln1_w;
    TD_TRY(td_norm_rows_launch(np, s));
    {  // fused q | k | v projection: q -> scratch, k | v -> kv_new
      TdGemmParams g = linear(f->xn, D, l.qkv_w, l.qkv_b, f->q, QW, n, QW + KVW, D);
      g.C2 = kv_new; g.ldc2 = KVW; g.n_split = QW;
      if (QW % 256 == 0) {
        // the column split needs a tile width that divides 256: every config but the 288x192 one
        g.cfg = n <= 32 ? -1 : (td_gemm_config_id(n, QW + KVW, D) == 1 ? 1 : 0);
        TD_TRY(run_linear(f, g, l.qkv_8, s));
      } else {
        TdGemmParams a = g; a.C2 = nullptr; a.N = QW;
        TD_TRY(td_gemm_launch(a, s));
        TdGemmParams b = a; b.W = l.qkv_w + (size_t)QW * D; b.bias = l.qkv_b + QW; b.N = KVW; b.C = kv_new; b.ldc = KVW;
        TD_TRY(td_gemm_launch(b, s));
      }
    }
    if (form.lora) TD_TRY(lora_add_qkv(f, li, kv_new, n, s));      // in front of RoPE
    TD_TRY(td_qk_norm_rope_launch(rq, s));
    rk.qkv = kv_new; TD_TRY(td_qk_norm_rope_launch(rk, s));
    if (kv8) {      // the quantising scatter runs BEFORE the attention, which then reads K^ | V^: no result depends on where a key came from
      const long long r0 = form.to_rows ? 0 : form.q8_cache_row0 + form.q8_tmp_row0;
      TD_TRY(td_kv_quant_rows_launch(kv_new, KVW, l.kv8 + (size_t)r0 * KVW, KVW, l.kvs + (size_t)r0 * 2 * Hkv, 2 * Hkv, kv_new, n, 2 * Hkv, form.to_rows, s));
      if (form.q8_stage_n > 0)
        TD_TRY(td_kv_dequant_rows_from_launch(l.kv8, KVW, l.kvs, 2 * Hkv, f->kvstage, KVW, form.q8_stage_n, 2 * Hkv, form.q8_stage_rows, s));
    } else if (form.to_rows)
      hipLaunchKernelGGL(td_kv_rows_to_rows_kernel, dim3((KVW / 8 + 255) / 256, n), dim3(256), 0, s, kv_new, l.kv, form.to_rows, KVW);
    else if (form.to_slots >= 0)
      hipLaunchKernelGGL(td_kv_rows_to_slots_kernel, dim3((KVW / 8 + 255) / 256, n), dim3(256), 0, s, kv_new, l.kv + form.to_slots, form.slots_L, f->slot_len, KVW);
    ap.K = kv8 ? (form.q8_stage_n > 0 ? f->kvstage : f->kvtmp) : form.attn_kv.of(f, l); ap.V = ap.K + Hkv * 128;
    TD_TRY(td_attn_launch(ap, s));
    // h += o_proj(attn)
    TD_TRY(run_linear(f, linear(f->attn, QW, l.o_w, nullptr, f->h, D, n, D, QW, true), l.o_8, s));
    if (form.lora) TD_TRY(lora_add_o(f, li, n, s));
    np.w = l.ln2_w;
    TD_TRY(td_norm_rows_launch(np, s));
    // gate | up, SwiGLU, down (+ residual)
    TD_TRY(run_linear(f, linear(f->xn, D, l.gu_w, nullptr, f->gu, 2 * I, n, 2 * I, D), l.gu_8, s));
    if (form.lora) TD_TRY(lora_add_gu(f, li, n, s));               // in front of SiLU * up
    TD_TRY(td_silu_mul_launch(f->gu, f->act, n, I, s));
    TD_TRY(run_linear(f, linear(f->act, I, l.down_w, nullptr, f->h, D, n, D, I, true), l.down_8, s));
    if (form.lora) TD_TRY(lora_add_down(f, li, n, s));
  }
  // model.norm -> captured embedding
  np.w = f->norm_w;
  TD_TRY(td_norm_rows_launch(np, s));
  if (hidden_out) TD_CHECK_HIP(hipMemcpyAsync(hidden_out, f->xn, (size_t)n * D * 2, hipMemcpyDeviceToDevice, s));
  return TD_OK;
}

// The part of a layer's attention descriptor every prefill form shares: q and the output in the engine's buffers, causal, 128-wide heads.
TdAttnParams prefill_attn(const td_qwen2* f, int batch, int Sq, int Skv, int causal_offset) {
  const int QW = f->Hq * 128;
  TdAttnParams ap;
  ap.Q = f->q; ap.ldq = QW; ap.ldkv = 2 * f->Hkv * 128; ap.O = f->attn; ap.ldo = QW;
  ap.batch = batch; ap.Sq = Sq; ap.Skv = Skv; ap.Hq = f->Hq; ap.Hkv = f->Hkv; ap.scale = 0.08838834764831845f;
  ap.causal = 1; ap.causal_offset = causal_offset;
  return ap;
}

}  // namespace

extern "C" {

// KV cache of n_slots sequences x slot_len rows per layer; activation workspace for slot_len rows (the longest prefill)
int td_qwen2_create_ex(const TdQwen2Config* cfg, int slot_len, int n_slots, int ws_rows, td_qwen2** out) {
  return td_qwen2_create_kv(cfg, slot_len, n_slots, ws_rows, TD_QWEN2_KV_BF16, out);
}

// ... with the KV cache in the given format: TD_QWEN2_KV_BF16 (td_qwen2_create_ex) or TD_QWEN2_KV_E4M3, in which every layer owns a byte plane and a scale
// plane instead of its bf16 rows (KVW + 8 Hkv bytes per row against 2 KVW)
int td_qwen2_create_kv(const TdQwen2Config* cfg, int slot_len, int n_slots, int ws_rows, int kv_mode, td_qwen2** out) {
  TD_CHECK_ARG(kv_mode == TD_QWEN2_KV_BF16 || kv_mode == TD_QWEN2_KV_E4M3, "td_qwen2_create_kv: unknown kv mode %d (TD_QWEN2_KV_BF16 = %d, TD_QWEN2_KV_E4M3 = %d)", kv_mode,
               TD_QWEN2_KV_BF16, TD_QWEN2_KV_E4M3);
  const bool kv8 = kv_mode == TD_QWEN2_KV_E4M3;
  TD_CHECK_ARG(cfg && out && slot_len > 0 && n_slots > 0 && (long long)slot_len * n_slots < (1ll << 30), "td_qwen2_create: bad arguments");
  if (ws_rows < slot_len) ws_rows = slot_len;
  const int max_tokens = slot_len * n_slots;
  TD_CHECK_ARG(cfg->head_dim == 128, "td_qwen2_create: head_dim must be 128");
  TD_CHECK_ARG((long long)max_tokens * 2 * cfg->num_kv_heads * 128 < (1ll << 31), "td_qwen2_create: %d cache rows of %d elements exceed the 32-bit row offsets of the decode step", max_tokens, 2 * cfg->num_kv_heads * 128);
  TD_CHECK_ARG(cfg->hidden % 512 == 0 && cfg->intermediate % 64 == 0, "td_qwen2_create: hidden %% 512 and intermediate %% 64 must be 0");
  TD_CHECK_ARG(cfg->num_heads % cfg->num_kv_heads == 0, "td_qwen2_create: heads must be a multiple of kv heads");
  TD_CHECK_ARG(cfg->mrope_section[0] + cfg->mrope_section[1] + cfg->mrope_section[2] == 64, "td_qwen2_create: mrope sections must sum to 64");
  td_qwen2* f = new td_qwen2();
  f->cfg = *cfg;
  const int D = f->D = cfg->hidden, I = f->I = cfg->intermediate;
  const int Hq = f->Hq = cfg->num_heads, Hkv = f->Hkv = cfg->num_kv_heads;
  const int NQKV = (Hq + 2 * Hkv) * 128;
  f->max_tokens = max_tokens;
  f->slot_len = slot_len;
  f->n_slots = n_slots;
  f->ws_rows = ws_rows;
  f->kv_mode = kv_mode;
  f->layers.resize(cfg->num_layers);

  int64_t off = 0, voff = 0;      // offset in this arena; offset in the arena of a bf16-mode handle (which holds the cache rows too)
  std::vector<std::pair<bf16_t**, int64_t>> fix;
  auto take = [&](bf16_t** p, int64_t n) {
    const int64_t padded = (n + 127) & ~int64_t(127);
    if (p) { fix.emplace_back(p, off); f->segs.push_back({off, voff, padded}); off += padded; }
    voff += padded;
  };
  take(&f->embed_w, (int64_t)cfg->vocab * D);
  take(&f->norm_w, D);
  if (!cfg->tie_embeddings) take(&f->lm_w, (int64_t)cfg->vocab * D);
  for (auto& l : f->layers) {
    take(&l.qkv_w, (int64_t)NQKV * D); take(&l.qkv_b, NQKV);
    take(&l.o_w, (int64_t)D * Hq * 128);
    take(&l.gu_w, (int64_t)2 * I * D);
    take(&l.down_w, (int64_t)D * I);
    take(&l.ln1_w, D); take(&l.ln2_w, D);
    take(kv8 ? nullptr : &l.kv, (int64_t)max_tokens * 2 * Hkv * 128);
  }
  f->arena_elems = off;
  hipError_t e = hipMalloc((void**)&f->arena, (size_t)off * 2);
  if (e != hipSuccess) {
    td_set_error("td_qwen2_create: hipMalloc of %.2f GiB failed: %s", off * 2.0 / (1 << 30), hipGetErrorString(e));
    delete f;
    return TD_ERR_HIP;
  }
  for (auto& fx : fix) *fx.first = f->arena + fx.second;
  if (cfg->tie_embeddings) f->lm_w = f->embed_w;
  if (kv8) {
    const int64_t plane = ((int64_t)max_tokens * 2 * Hkv * 128 + 255) & ~int64_t(255), splane = ((int64_t)max_tokens * 2 * Hkv * 4 + 255) & ~int64_t(255);
    const int64_t bytes = (plane + splane) * cfg->num_layers;
    e = hipMalloc((void**)&f->kv8_arena, (size_t)bytes);
    if (e != hipSuccess) {
      td_set_error("td_qwen2_create_kv: hipMalloc of %.2f GiB for the e4m3 cache failed: %s", bytes / double(1 << 30), hipGetErrorString(e));
      (void)hipFree(f->arena);
      delete f;
      return TD_ERR_HIP;
    }
    e = hipMemset(f->kv8_arena, 0, (size_t)bytes);      // (ordered with every stream by the synchronise below)
    if (e != hipSuccess) {
      td_set_error("td_qwen2_create_kv: hipMemset of the e4m3 cache failed: %s", hipGetErrorString(e));
      (void)hipFree(f->kv8_arena);
      (void)hipFree(f->arena);
      delete f;
      return TD_ERR_HIP;
    }
    int64_t o = 0;
    for (auto& l : f->layers) {
      l.kv8 = (uint8_t*)(f->kv8_arena + o); o += plane;
      l.kvs = (float*)(f->kv8_arena + o); o += splane;
    }
  }

  q_add(f, "model.embed_tokens.weight", f->embed_w, (int64_t)cfg->vocab * D);
  q_add(f, "model.norm.weight", f->norm_w, D);
  if (!cfg->tie_embeddings) q_add(f, "lm_head.weight", f->lm_w, (int64_t)cfg->vocab * D);
  for (int i = 0; i < cfg->num_layers; ++i) {
    QLayer& l = f->layers[i];
    const std::string p = "model.layers." + std::to_string(i) + ".";
    q_add(f, p + "self_attn.q_proj.weight", l.qkv_w, (int64_t)Hq * 128 * D);
    q_add(f, p + "self_attn.q_proj.bias", l.qkv_b, Hq * 128);
    q_add(f, p + "self_attn.k_proj.weight", l.qkv_w + (int64_t)Hq * 128 * D, (int64_t)Hkv * 128 * D);
    q_add(f, p + "self_attn.k_proj.bias", l.qkv_b + Hq * 128, Hkv * 128);
    q_add(f, p + "self_attn.v_proj.weight", l.qkv_w + (int64_t)(Hq + Hkv) * 128 * D, (int64_t)Hkv * 128 * D);
    q_add(f, p + "self_attn.v_proj.bias", l.qkv_b + (Hq + Hkv) * 128, Hkv * 128);
    q_add(f, p + "self_attn.o_proj.weight", l.o_w, (int64_t)D * Hq * 128);
    q_add(f, p + "mlp.gate_proj.weight", l.gu_w, (int64_t)I * D);
    q_add(f, p + "mlp.up_proj.weight", l.gu_w + (int64_t)I * D, (int64_t)I * D);
    q_add(f, p + "mlp.down_proj.weight", l.down_w, (int64_t)D * I);
    q_add(f, p + "input_layernorm.weight", l.ln1_w, D);
    q_add(f, p + "post_attention_layernorm.weight", l.ln2_w, D);
  }

  const int64_t n = ws_rows;
  struct Req { void** p; int64_t bytes; };
  std::vector<Req> reqs = {
      {(void**)&f->h, n * D * 2}, {(void**)&f->xn, n * D * 2}, {(void**)&f->q, n * Hq * 128 * 2},
      {(void**)&f->attn, n * Hq * 128 * 2}, {(void**)&f->gu, n * 2 * I * 2}, {(void**)&f->act, n * I * 2},
      {(void**)&f->cosT, n * 128 * 4}, {(void**)&f->sinT, n * 128 * 4},
      {(void**)&f->kvtmp, n * 2 * Hkv * 128 * 2}, {(void**)&f->ibuf, (7 * MAX_BATCH + 16) * 4}, {(void**)&f->lastrows, (int64_t)MAX_BATCH * D * 2},
      {(void**)&f->tok_buf, MAX_BATCH * 4}, {(void**)&f->pos_buf, 3 * MAX_BATCH * 4}, {(void**)&f->logits_buf, (int64_t)MAX_BATCH * cfg->vocab * 2},
      {(void**)&f->sk_ws, SK_WS_BYTES}, {(void**)&f->row_map, n * 4},
  };
  int64_t total = 0;
  for (auto& r : reqs) total += (r.bytes + 255) & ~int64_t(255);
  e = hipMalloc((void**)&f->ws, (size_t)total);
  if (e != hipSuccess) {
    td_set_error("td_qwen2_create: hipMalloc of %.2f GiB workspace failed: %s", total / double(1 << 30), hipGetErrorString(e));
    (void)hipFree(f->arena);
    if (f->kv8_arena) (void)hipFree(f->kv8_arena);
    delete f;
    return TD_ERR_HIP;
  }
  (void)hipMemset(f->ws, 0, (size_t)total);
  (void)hipDeviceSynchronize();   // the handle may be used from any stream next; a null-stream memset is not ordered with non-blocking streams
  int64_t o = 0;
  for (auto& r : reqs) { *r.p = f->ws + o; o += (r.bytes + 255) & ~int64_t(255); }
  *out = f;
  return TD_OK;
}

static void drop_step_graphs(td_qwen2* f) {
  for (auto& kv : f->step_graphs) (void)hipGraphExecDestroy(kv.second);
  f->step_graphs.clear();
  f->step_calls.clear();
}

void td_qwen2_destroy(td_qwen2* f) {
  if (!f) return;
  drop_step_graphs(f);
  if (f->capture_stream) (void)hipStreamDestroy(f->capture_stream);
  (void)hipFree(f->arena);
  (void)hipFree(f->ws);
  if (f->w8_arena) (void)hipFree(f->w8_arena);
  if (f->kv8_arena) (void)hipFree(f->kv8_arena);
  if (f->kvstage) (void)hipFree(f->kvstage);
  if (f->lora_arena) (void)hipFree(f->lora_arena);
  delete f;
}

int td_qwen2_kv_info(const td_qwen2* f, int* kv_mode, int64_t* bytes_per_row, int64_t* cache_bytes) {
  TD_CHECK_ARG(f, "td_qwen2_kv_info: null handle");
  const int64_t KVW = (int64_t)2 * f->Hkv * 128;
  const int64_t row = f->kv_mode == TD_QWEN2_KV_E4M3 ? KVW + 8 * f->Hkv : 2 * KVW;      // bytes + 2 Hkv fp32 scales | bf16
  if (kv_mode) *kv_mode = f->kv_mode;
  if (bytes_per_row) *bytes_per_row = row;
  if (cache_bytes) *cache_bytes = row * f->max_tokens * f->cfg.num_layers;
  return TD_OK;
}

// rows [row0, row0 + n) of sequence `slot` in layer `layer` as bf16 [n, 2 Hkv 128]: a copy, or -- e4m3 cache -- the dequantised values q 2^e (exact)
int td_qwen2_read_kv(td_qwen2* f, int layer, int slot, int row0, int n, void* out_bf16, void* stream) {
  TD_CHECK_ARG(f && out_bf16, "td_qwen2_read_kv: null argument");
  TD_CHECK_ARG(layer >= 0 && layer < f->cfg.num_layers && slot >= 0 && slot < f->n_slots, "td_qwen2_read_kv: layer %d of %d, slot %d of %d", layer, f->cfg.num_layers, slot, f->n_slots);
  TD_CHECK_ARG(row0 >= 0 && n > 0 && (long long)row0 + n <= f->slot_len, "td_qwen2_read_kv: rows [%d, %lld) exceed the slot capacity %d", row0, (long long)row0 + n, f->slot_len);
  TD_CHECK_ARG((uintptr_t)out_bf16 % 16 == 0, "td_qwen2_read_kv: the output must be 16-byte aligned");
  const QLayer& l = f->layers[layer];
  const size_t KVW = (size_t)2 * f->Hkv * 128, r = (size_t)slot * f->slot_len + row0;
  if (f->kv_mode == TD_QWEN2_KV_E4M3)
    return td_kv_dequant_rows_launch(l.kv8 + r * KVW, (long long)KVW, l.kvs + r * 2 * f->Hkv, 2 * f->Hkv, (bf16_t*)out_bf16, (long long)KVW, n, 2 * f->Hkv, (hipStream_t)stream);
  TD_CHECK_HIP(hipMemcpyAsync(out_bf16, l.kv + r * KVW, (size_t)n * KVW * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

int td_qwen2_quantize_weights(td_qwen2* f, int mode, void* stream) {
  TD_CHECK_ARG(f, "td_qwen2_quantize_weights: null handle");
  TD_CHECK_ARG(mode == TD_QWEN2_WEIGHTS_E4M3 || mode == TD_QWEN2_WEIGHTS_MXFP4,
               "td_qwen2_quantize_weights: unknown mode %d (TD_QWEN2_WEIGHTS_E4M3 = %d and TD_QWEN2_WEIGHTS_MXFP4 = %d are the ones served)", mode, TD_QWEN2_WEIGHTS_E4M3,
               TD_QWEN2_WEIGHTS_MXFP4);
  const bool mx4 = mode == TD_QWEN2_WEIGHTS_MXFP4;
  TD_CHECK_ARG(f->w_mode != TD_QWEN2_WEIGHTS_INT4,
               "td_qwen2_quantize_weights: the handle holds AWQ / GPTQ int4 weights (TD_QWEN2_WEIGHTS_INT4), and one handle holds one weight format: its decoder "
               "Linears came quantised and are not quantised again");
  // the arena holds W^ of the mode it was quantised in, not the weights it was loaded with: another format would quantise the wrong model
  TD_CHECK_ARG(f->w_mode == TD_QWEN2_WEIGHTS_BF16 || f->w_mode == mode || f->w8_stale,
               "td_qwen2_quantize_weights: the handle was quantised as %s and its original weights are gone; load its parameters again before quantising as %s",
               f->w_mode == TD_QWEN2_WEIGHTS_MXFP4 ? "TD_QWEN2_WEIGHTS_MXFP4" : "TD_QWEN2_WEIGHTS_E4M3", mx4 ? "TD_QWEN2_WEIGHTS_MXFP4" : "TD_QWEN2_WEIGHTS_E4M3");
  const int D = f->D, I = f->I, QW = f->Hq * 128, NQKV = (f->Hq + 2 * f->Hkv) * 128;
  struct Lin { bf16_t* w; W8Ref* ref; int N, K; };
  std::vector<Lin> lins;
  for (QLayer& l : f->layers) {
    lins.push_back({l.qkv_w, &l.qkv_8, NQKV, D});
    lins.push_back({l.o_w, &l.o_8, D, QW});
    lins.push_back({l.gu_w, &l.gu_8, 2 * I, D});
    lins.push_back({l.down_w, &l.down_8, D, I});
  }
  lins.push_back({f->lm_w, &f->lm_8, f->cfg.vocab, D});      // (tied embeddings: this is the embedding table)
  if (mx4)
    for (const Lin& x : lins) TD_CHECK_ARG(x.K % 32 == 0, "td_qwen2_quantize_weights: TD_QWEN2_WEIGHTS_MXFP4 needs every Linear's K=%d to be a multiple of 32 (one MX block)", x.K);
  if (f->w8_arena && f->w_mode != mode) {      // reloaded and quantised in the other format: its copy has other sizes
    (void)hipFree(f->w8_arena);
    f->w8_arena = nullptr;
  }
  // bytes of a Linear's weight piece and of its scale piece
  auto wbytes = [&](const Lin& x) { return mx4 ? (int64_t)x.N * x.K / 2 : (int64_t)x.N * x.K; };
  auto sbytes = [&](const Lin& x) { return mx4 ? (int64_t)x.N * x.K / 32 : (int64_t)x.N * 4; };
  if (!f->w8_arena) {
    int64_t total = 0;
    for (const Lin& x : lins) total += ((wbytes(x) + 255) & ~int64_t(255)) + ((sbytes(x) + 255) & ~int64_t(255));
    hipError_t e = hipMalloc((void**)&f->w8_arena, (size_t)total);
    if (e != hipSuccess) {
      f->w8_arena = nullptr;
      td_set_error("td_qwen2_quantize_weights: hipMalloc of %.2f GiB for the quantised copy failed: %s", total / double(1 << 30), hipGetErrorString(e));
      return TD_ERR_HIP;
    }
    int64_t o = 0;
    for (const Lin& x : lins) {
      x.ref->q = (uint8_t*)(f->w8_arena + o); o += (wbytes(x) + 255) & ~int64_t(255);
      x.ref->s = f->w8_arena + o; o += (sbytes(x) + 255) & ~int64_t(255);
    }
    f->w8_bytes = 0;
    for (const Lin& x : lins) f->w8_bytes += wbytes(x) + sbytes(x);      // (reported without the padding between the pieces)
    f->w8_linears = (int)lins.size();
  }
  drop_step_graphs(f);      // the captured steps carry the bf16 launch list
  f->w8_stale = true;       // (a failing launch below must not leave a half-quantised handle runnable)
  f->w_mode = mode;
  for (const Lin& x : lins) {
    if (mx4) TD_TRY(td_quant_weight_rows_mxfp4_launch(x.w, x.K, x.ref->q, (uint8_t*)x.ref->s, x.w, x.N, x.K, (hipStream_t)stream));
    else TD_TRY(td_quant_weight_rows_launch(x.w, x.K, x.ref->q, (float*)x.ref->s, x.w, x.N, x.K, (hipStream_t)stream));
  }
  f->w8_stale = false;
  f->w8_on = true;
  return TD_OK;
}

int td_qwen2_set_weight_stream(td_qwen2* f, int on) {
  TD_CHECK_ARG(f, "td_qwen2_set_weight_stream: null handle");
  TD_CHECK_ARG(f->w_mode != TD_QWEN2_WEIGHTS_BF16, "td_qwen2_set_weight_stream: the handle is not quantised (td_qwen2_quantize_weights first)");
  const int prev = f->w8_on ? 1 : 0;
  f->w8_on = on != 0;
  drop_step_graphs(f);      // the captured steps carry the old launch list
  return prev;
}

int td_qwen2_set_int4_routing(td_qwen2* f, int all) {
  TD_CHECK_ARG(all == 0 || all == 1, "td_qwen2_set_int4_routing: all=%d: 0 (the measured row counts) or 1 (every row count the int4 forms take)", all);
  TD_CHECK_ARG(f, "td_qwen2_set_int4_routing: null handle");
  TD_CHECK_ARG(f->w_mode == TD_QWEN2_WEIGHTS_INT4, "td_qwen2_set_int4_routing: the handle holds no int4 weights (td_qwen2_load_param_int4 first)");
  const int prev = f->i4_route_all ? 1 : 0;
  f->i4_route_all = all != 0;
  drop_step_graphs(f);      // the captured steps carry the old launch list
  return prev;
}

int64_t td_qwen2_weight_stream_launches(const td_qwen2* f) { return f ? (int64_t)f->w8_launches : -1; }

int td_qwen2_weight_info(const td_qwen2* f, int* mode, int* stream_on, int64_t* bytes_8bit, int* n_linears) {
  TD_CHECK_ARG(f, "td_qwen2_weight_info: null handle");
  if (mode) *mode = f->w_mode;
  if (stream_on) *stream_on = f->w8_on ? 1 : 0;
  if (bytes_8bit) *bytes_8bit = f->w8_bytes;
  if (n_linears) *n_linears = f->w8_linears;
  return TD_OK;
}

int td_qwen2_num_params(const td_qwen2* f) { return f ? (int)f->slots.size() : 0; }

int td_qwen2_param_info(const td_qwen2* f, int idx, char* name_buf, int buf_len, int64_t* count) {
  TD_CHECK_ARG(f && idx >= 0 && idx < (int)f->slots.size(), "td_qwen2_param_info: index %d out of range", idx);
  if (name_buf && buf_len > 0) {
    strncpy(name_buf, f->slots[idx].name.c_str(), buf_len - 1);
    name_buf[buf_len - 1] = 0;
  }
  if (count) *count = f->slots[idx].count;
  return TD_OK;
}

namespace {
// Is slot `s` one of the 7 x layers decoder Linear weights a checkpoint quantises?  Then: its layer, which of q, k, v, o, gate, up, down it is, its extents,
// its first row in the fused Linear the engine runs (q|k|v and gate|up are row concatenations) and that Linear's copy.
bool int4_linear_of(td_qwen2* f, const QSlot& s, int* layer, int* which, int* N, int* K, int* row0, W8Ref** ref) {
  const int D = f->D, I = f->I, QW = f->Hq * 128, KVW = f->Hkv * 128;
  for (int i = 0; i < (int)f->layers.size(); ++i) {
    QLayer& l = f->layers[i];
    struct Cand { bf16_t* p; int N, K, row0; W8Ref* ref; };
    const Cand c[7] = {{l.qkv_w, QW, D, 0, &l.qkv_8}, {l.qkv_w + (int64_t)QW * D, KVW, D, QW, &l.qkv_8}, {l.qkv_w + (int64_t)(QW + KVW) * D, KVW, D, QW + KVW, &l.qkv_8},
                       {l.o_w, D, QW, 0, &l.o_8}, {l.gu_w, I, D, 0, &l.gu_8}, {l.gu_w + (int64_t)I * D, I, D, I, &l.gu_8}, {l.down_w, D, I, 0, &l.down_8}};
    for (int w = 0; w < 7; ++w)
      if (s.ptr == c[w].p && s.count == (int64_t)c[w].N * c[w].K) {
        *layer = i; *which = w; *N = c[w].N; *K = c[w].K; *row0 = c[w].row0; *ref = c[w].ref;
        return true;
      }
  }
  return false;
}
}  // namespace

int td_qwen2_load_param_int4(td_qwen2* f, const char* name, const void* packed, const void* scales, const void* zeros, int G, void* stream) {
  TD_CHECK_ARG(G == 32 || G == 64 || G == 128, "td_qwen2_load_param_int4: G=%d: the group sizes served are 32, 64 and 128", G);
  TD_CHECK_ARG(f && name && packed && scales && zeros, "td_qwen2_load_param_int4: the handle, name, packed, scales and zeros are required");
  TD_CHECK_ARG((uintptr_t)packed % 4 == 0 && (uintptr_t)scales % 2 == 0, "td_qwen2_load_param_int4: misaligned operands: packed must be 4-byte aligned, scales 2-byte");
  TD_CHECK_ARG(f->w_mode == TD_QWEN2_WEIGHTS_BF16 || f->w_mode == TD_QWEN2_WEIGHTS_INT4,
               "td_qwen2_load_param_int4: the handle was quantised as %s, and one handle holds one weight format: create another handle for an AWQ / GPTQ checkpoint",
               f->w_mode == TD_QWEN2_WEIGHTS_MXFP4 ? "TD_QWEN2_WEIGHTS_MXFP4" : "TD_QWEN2_WEIGHTS_E4M3");
  TD_CHECK_ARG(f->i4_G == 0 || f->i4_G == G, "td_qwen2_load_param_int4: G=%d, but the handle holds int4 weights of group size %d: one handle, one group size", G, f->i4_G);
  auto it = f->index.find(name);
  TD_CHECK_ARG(it != f->index.end(), "td_qwen2_load_param_int4: unknown parameter '%s'", name);
  const QSlot& s = f->slots[it->second];
  int layer, which, N, K, row0;
  W8Ref* ref;
  TD_CHECK_ARG(int4_linear_of(f, s, &layer, &which, &N, &K, &row0, &ref),
               "td_qwen2_load_param_int4: '%s' is not a decoder Linear weight (q / k / v / o / gate / up / down_proj.weight); everything else loads as bf16", name);
  const int D = f->D, I = f->I, QW = f->Hq * 128, NQKV = (f->Hq + 2 * f->Hkv) * 128;
  TD_CHECK_ARG(D % G == 0 && I % G == 0 && D % 32 == 0 && I % 32 == 0,
               "td_qwen2_load_param_int4: G=%d must divide hidden=%d and intermediate=%d (and both must be multiples of 32, one 16-byte chunk of a packed row)", G, D, I);
  if (!f->w8_arena) {      // the copy of all 4 x layers fused Linears, from their shapes
    struct Lin { W8Ref* ref; int N, K; };
    std::vector<Lin> lins;
    for (QLayer& l : f->layers) {
      lins.push_back({&l.qkv_8, NQKV, D});
      lins.push_back({&l.o_8, D, QW});
      lins.push_back({&l.gu_8, 2 * I, D});
      lins.push_back({&l.down_8, D, I});
    }
    auto pad = [](int64_t b) { return (b + 255) & ~int64_t(255); };
    int64_t total = 0, bytes = 0;
    for (const Lin& x : lins) {
      const int64_t w = (int64_t)x.N * x.K / 2, g = (int64_t)x.N * (x.K / G);
      total += pad(w) + pad(2 * g) + pad(g);
      bytes += w + 3 * g;
    }
    hipError_t e = hipMalloc((void**)&f->w8_arena, (size_t)total);
    if (e != hipSuccess) {
      f->w8_arena = nullptr;
      td_set_error("td_qwen2_load_param_int4: hipMalloc of %.2f GiB for the int4 copy failed: %s", total / double(1 << 30), hipGetErrorString(e));
      return TD_ERR_HIP;
    }
    int64_t o = 0;
    for (const Lin& x : lins) {
      const int64_t w = (int64_t)x.N * x.K / 2, g = (int64_t)x.N * (x.K / G);
      x.ref->q = (uint8_t*)(f->w8_arena + o); o += pad(w);
      x.ref->s = f->w8_arena + o; o += pad(2 * g);
      x.ref->z = (uint8_t*)(f->w8_arena + o); o += pad(g);
    }
    f->w8_bytes = bytes;      // (reported without the padding between the pieces)
    f->w8_linears = 7 * (int)f->layers.size();
    f->i4_have.assign((size_t)f->w8_linears, 0);
    f->i4_loaded = 0;
    f->i4_G = G;
    f->w8_on = false;
  }
  drop_step_graphs(f);
  f->w_mode = TD_QWEN2_WEIGHTS_INT4;
  const bool was_whole = f->i4_loaded == (int)f->i4_have.size();
  f->w8_stale = true;      // (a failing call below must not leave a half-loaded handle runnable)
  const int ng = K / G;
  uint8_t* dq = ref->q + (size_t)row0 * (K / 2);
  uint16_t* ds = (uint16_t*)ref->s + (size_t)row0 * ng;
  uint8_t* dz = ref->z + (size_t)row0 * ng;
  TD_CHECK_HIP(hipMemcpyAsync(dq, packed, (size_t)N * (K / 2), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  TD_CHECK_HIP(hipMemcpyAsync(ds, scales, (size_t)N * ng * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  TD_CHECK_HIP(hipMemcpyAsync(dz, zeros, (size_t)N * ng, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  TD_TRY(td_dequant_rows_int4_launch(dq, ds, dz, G, s.ptr, K, N, K, (hipStream_t)stream));      // W^ from the copy itself: the arena is what the stream reads
  char& have = f->i4_have[(size_t)layer * 7 + which];
  if (!have) { have = 1; ++f->i4_loaded; }
  if (f->i4_loaded == (int)f->i4_have.size()) {
    f->w8_stale = false;
    if (!was_whole) f->w8_on = true;
  }
  return TD_OK;
}

int td_qwen2_load_param(td_qwen2* f, const char* name, const void* src, int64_t count, void* stream) {
  TD_CHECK_ARG(f && name && src, "td_qwen2_load_param: null argument");
  auto it = f->index.find(name);
  TD_CHECK_ARG(it != f->index.end(), "td_qwen2_load_param: unknown parameter '%s'", name);
  const QSlot& s = f->slots[it->second];
  TD_CHECK_ARG(s.count == count, "td_qwen2_load_param: '%s' expects %lld elements, got %lld", name, (long long)s.count, (long long)count);
  if (f->w_mode == TD_QWEN2_WEIGHTS_INT4) {      // biases, norms, embeddings and lm_head have no int4 copy: they load as ever and leave the handle as it is
    int layer, which, N, K, row0;
    W8Ref* ref;
    TD_CHECK_ARG(!int4_linear_of(f, s, &layer, &which, &N, &K, &row0, &ref),
                 "td_qwen2_load_param: '%s' is a decoder Linear of a handle that holds int4 weights (TD_QWEN2_WEIGHTS_INT4), and one handle holds one weight format: "
                 "load it through td_qwen2_load_param_int4, or create another handle for bf16 weights", name);
    TD_CHECK_HIP(hipMemcpyAsync(s.ptr, src, (size_t)count * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TD_OK;
  }
  TD_CHECK_HIP(hipMemcpyAsync(s.ptr, src, (size_t)count * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (f->w_mode != TD_QWEN2_WEIGHTS_BF16) f->w8_stale = true;      // the 8-bit copy no longer matches: td_qwen2_quantize_weights again
  return TD_OK;
}

int td_qwen2_init_random(td_qwen2* f, uint64_t seed, float std, void* stream) {
  TD_CHECK_ARG(f, "td_qwen2_init_random: null handle");
  TD_CHECK_ARG(f->w_mode != TD_QWEN2_WEIGHTS_INT4, "td_qwen2_init_random: the handle holds int4 weights (TD_QWEN2_WEIGHTS_INT4), and one handle holds one weight "
               "format: random bf16 weights over its decoder Linears would leave the int4 copy behind");
  if (f->w_mode != TD_QWEN2_WEIGHTS_BF16) f->w8_stale = true;
  if (f->kv_mode == TD_QWEN2_KV_BF16) {
    TD_TRY(td_fill_normal_bf16(f->arena, f->arena_elems, seed, std, 0.f, stream));
  } else {      // the arena lacks the cache rows: every piece draws what it draws at its place in a bf16-mode handle (pieces start on even offsets)
    for (const td_qwen2::Seg& g : f->segs) TD_TRY(td_fill_normal_from_launch(f->arena + g.off, g.n, seed, std, 0.f, g.voff / 2, (hipStream_t)stream));
  }
  for (const QSlot& s : f->slots)
    if (s.name.find("layernorm.weight") != std::string::npos || s.name == "model.norm.weight")
      TD_TRY(td_fill_normal_bf16(s.ptr, s.count, seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(f->voff_of(s.ptr) + 1)), 0.05f, 1.0f, stream));
  return TD_OK;
}

// out[i,:] = embed_tokens[ids[i],:] -- the host builds `inputs_embeds` from this, replacing the image-placeholder
// rows with the vision tower's merged tokens ([ext] Qwen2VLModel.forward masked_scatter).
int td_qwen2_embed_tokens(td_qwen2* f, const int* token_ids, void* out, int n, void* stream) {
  TD_CHECK_ARG(f && token_ids && out && n > 0, "td_qwen2_embed_tokens: null argument");
  TD_QWEN2_FRESH(f, "td_qwen2_embed_tokens");      // (with tied embeddings the table is a quantised weight; untied handles are refused too: one rule)
  return td_embed_gather_launch(token_ids, f->embed_w, (bf16_t*)out, n, f->D, f->cfg.vocab, (hipStream_t)stream);
}

// Runs n new tokens at cache positions [pos0, pos0 + n) of sequence `slot` through the decoder.
//   token_ids  : device int32 [n], or NULL when inputs_embeds is given
//   inputs_embeds : device bf16 [n, hidden] (token embeddings with the image-token rows replaced by the
//                vision tower's output), or NULL
//   position_ids : device int32 [3, n] M-RoPE streams (temporal, height, width); text tokens repeat one value
//   hidden_out : device bf16 [n, hidden] = model.norm(h)  -- the embedding the reference captures
//                ("embedding_layer_name: model.norm"); may be NULL
//   logits_last: device bf16 [vocab] for the LAST of the n tokens (lm_head), or NULL
int td_qwen2_forward_slot(td_qwen2* f, int slot, const int* token_ids, const void* inputs_embeds, const int* position_ids, int n,
                          int pos0, void* hidden_out, void* logits_last, void* stream) {
  TD_CHECK_ARG(f && position_ids && (token_ids || inputs_embeds), "td_qwen2_forward: null argument");
  TD_QWEN2_FRESH(f, "td_qwen2_forward");
  TD_CHECK_ARG(slot >= 0 && slot < f->n_slots, "td_qwen2_forward: slot %d outside the %d configured sequences", slot, f->n_slots);
  TD_CHECK_ARG(n > 0 && pos0 >= 0 && pos0 + n <= f->slot_len, "td_qwen2_forward: positions [%d, %d) exceed the cache capacity %d", pos0, pos0 + n, f->slot_len);
  hipStream_t s = (hipStream_t)stream;
  const long long KVW = 2 * f->Hkv * 128, seq = (long long)slot * f->slot_len * KVW;   // this sequence's cache rows
  PrefillForm form;
  form.n = n;
  form.attn = prefill_attn(f, 1, n, pos0 + n, pos0);
  if (f->kv_mode == TD_QWEN2_KV_E4M3) {
    // staging: the slot's rows [0, pos0) are dequantised into kvtmp, the new rows join them there, the bf16 attention runs over kvtmp (ws_rows >= slot_len rows)
    form.q8_tmp_row0 = pos0; form.q8_cache_row0 = (long long)slot * f->slot_len;
  } else {
    form.kv_new = KvRows{seq + pos0 * KVW};      // k | v -> straight into the layer's cache rows
    form.attn_kv = KvRows{seq};
  }
  if (f->lora_max > 0) {
    int rc;
    f->lora_rows_host.assign((size_t)n, f->slot_adapter(slot));
    form.lora = lora_upload_rows(f, n, s, &rc);
    TD_TRY(rc);
  }
  TD_TRY(prefill_pass(f, form, token_ids, inputs_embeds, position_ids, hidden_out, s));
  if (logits_last) TD_TRY(lm_head(f, f->xn + (size_t)(n - 1) * f->D, 1, logits_last, s));
  return TD_OK;
}

// ... of the first (or only) sequence
int td_qwen2_forward(td_qwen2* f, const int* token_ids, const void* inputs_embeds, const int* position_ids, int n,
                     int pos0, void* hidden_out, void* logits_last, void* stream) {
  return td_qwen2_forward_slot(f, 0, token_ids, inputs_embeds, position_ids, n, pos0, hidden_out, logits_last, stream);
}

int td_qwen2_create_slots(const TdQwen2Config* cfg, int slot_len, int n_slots, td_qwen2** out) { return td_qwen2_create_ex(cfg, slot_len, n_slots, slot_len, out); }
int td_qwen2_create(const TdQwen2Config* cfg, int max_tokens, td_qwen2** out) { return td_qwen2_create_ex(cfg, max_tokens, 1, max_tokens, out); }

// re-partition the cache rows; a sequence cannot be longer than the activation workspace the handle was created with
int td_qwen2_set_slots(td_qwen2* f, int n_slots) {
  TD_CHECK_ARG(f && n_slots >= 1 && n_slots <= f->max_tokens, "td_qwen2_set_slots: bad slot count %d", n_slots);
  f->n_slots = n_slots;
  f->slot_len = f->max_tokens / n_slots < f->ws_rows ? f->max_tokens / n_slots : f->ws_rows;
  f->slot_lora.clear();     // the slots are other cache rows now: none carries an adapter
  drop_step_graphs(f);      // the captured steps carry the old slot stride
  return TD_OK;
}

int td_qwen2_set_fused_rope(td_qwen2* f, int on) {
  TD_CHECK_ARG(f, "td_qwen2_set_fused_rope: null handle");
  const int prev = f->fused_rope ? 1 : 0;
  f->fused_rope = on != 0;
  drop_step_graphs(f);      // the captured steps carry the old launch list
  return prev;
}

int td_qwen2_slot_capacity(const td_qwen2* f) { return f ? f->slot_len : 0; }

int td_qwen2_move_slot(td_qwen2* f, int src, int dst, int len, void* stream) {
  TD_CHECK_ARG(f && src >= 0 && src < f->n_slots && dst >= 0 && dst < f->n_slots && len >= 0 && len <= f->slot_len, "td_qwen2_move_slot: bad arguments");
  if (src != dst && f->lora_max > 0) {      // the destination continues the source's sequence: under its adapter
    if ((int)f->slot_lora.size() <= dst) f->slot_lora.resize((size_t)dst + 1, -1);
    f->slot_lora[(size_t)dst] = f->slot_adapter(src);
  }
  if (src == dst || len == 0) return TD_OK;
  const size_t KVW = (size_t)2 * f->Hkv * 128;
  if (f->kv_mode == TD_QWEN2_KV_E4M3) {      // both planes
    const size_t SW = (size_t)2 * f->Hkv;
    for (const QLayer& l : f->layers) {
      TD_CHECK_HIP(hipMemcpyAsync(l.kv8 + (size_t)dst * f->slot_len * KVW, l.kv8 + (size_t)src * f->slot_len * KVW, (size_t)len * KVW, hipMemcpyDeviceToDevice, (hipStream_t)stream));
      TD_CHECK_HIP(hipMemcpyAsync(l.kvs + (size_t)dst * f->slot_len * SW, l.kvs + (size_t)src * f->slot_len * SW, (size_t)len * SW * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return TD_OK;
  }
  for (const QLayer& l : f->layers)
    TD_CHECK_HIP(hipMemcpyAsync(l.kv + (size_t)dst * f->slot_len * KVW, l.kv + (size_t)src * f->slot_len * KVW, (size_t)len * KVW * 2,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

// one launch for every plane and destination (td_kv_fork_rows): n sequences continuing from one prefill
int td_qwen2_fork_slot(td_qwen2* f, int src, const int* dst_slots, int n_dst, int len, void* stream) {
  TD_CHECK_ARG(f, "td_qwen2_fork_slot: null handle");
  TD_CHECK_ARG(dst_slots, "td_qwen2_fork_slot: null dst_slots");
  TD_CHECK_ARG(n_dst >= 1, "td_qwen2_fork_slot: n_dst=%d, at least one destination is needed", n_dst);
  TD_CHECK_ARG(src >= 0 && src < f->n_slots, "td_qwen2_fork_slot: source slot %d outside the %d configured sequences", src, f->n_slots);
  for (int i = 0; i < n_dst; ++i)
    TD_CHECK_ARG(dst_slots[i] >= 0 && dst_slots[i] < f->n_slots, "td_qwen2_fork_slot: destination slot %d outside the %d configured sequences", dst_slots[i], f->n_slots);
  TD_CHECK_ARG(len >= 0 && len <= f->slot_len, "td_qwen2_fork_slot: len=%d exceeds the slot capacity %d", len, f->slot_len);
  if (f->lora_max > 0)
    for (int i = 0; i < n_dst; ++i) {      // every destination continues the source's sequence: under its adapter
      if ((int)f->slot_lora.size() <= dst_slots[i]) f->slot_lora.resize((size_t)dst_slots[i] + 1, -1);
      f->slot_lora[(size_t)dst_slots[i]] = f->slot_adapter(src);
    }
  const int64_t KVW = (int64_t)2 * f->Hkv * 128, SW = (int64_t)2 * f->Hkv;
  std::vector<TdKvPlane> planes;
  for (const QLayer& l : f->layers) {
    if (f->kv_mode == TD_QWEN2_KV_E4M3) {
      planes.push_back(TdKvPlane{l.kv8, KVW, f->slot_len});
      planes.push_back(TdKvPlane{l.kvs, SW * 4, f->slot_len});
    } else {
      planes.push_back(TdKvPlane{l.kv, KVW * 2, f->slot_len});
    }
  }
  return td_kv_fork_rows(planes.data(), (int)planes.size(), src, dst_slots, n_dst, len, stream);
}

// the reordering of a beam-search step (td_kv_gather_rows): row j takes the cache rows of row copy_src_dev[j], which only the device knows
int td_qwen2_gather_slots(td_qwen2* f, int n, const int* slots, const int32_t* copy_src_dev, const int* lens, void* stream) {
  TD_CHECK_ARG(f, "td_qwen2_gather_slots: null handle");
  TD_CHECK_ARG(slots, "td_qwen2_gather_slots: null slots");
  TD_CHECK_ARG(copy_src_dev, "td_qwen2_gather_slots: null copy_src_dev");
  TD_CHECK_ARG(lens, "td_qwen2_gather_slots: null lens");
  TD_CHECK_ARG(n >= 1 && n <= 256, "td_qwen2_gather_slots: n=%d rows outside 1..256", n);
  for (int j = 0; j < n; ++j) {
    TD_CHECK_ARG(slots[j] >= 0 && slots[j] < f->n_slots, "td_qwen2_gather_slots: slot %d of row %d outside the %d configured sequences", slots[j], j, f->n_slots);
    TD_CHECK_ARG(lens[j] >= 0 && lens[j] <= f->slot_len, "td_qwen2_gather_slots: len=%d of row %d exceeds the slot capacity %d", lens[j], j, f->slot_len);
  }
  const int64_t KVW = (int64_t)2 * f->Hkv * 128, SW = (int64_t)2 * f->Hkv;
  std::vector<TdKvPlane> planes;
  for (const QLayer& l : f->layers) {
    if (f->kv_mode == TD_QWEN2_KV_E4M3) {
      planes.push_back(TdKvPlane{l.kv8, KVW, f->slot_len});
      planes.push_back(TdKvPlane{l.kvs, SW * 4, f->slot_len});
    } else {
      planes.push_back(TdKvPlane{l.kv, KVW * 2, f->slot_len});
    }
  }
  return td_kv_gather_rows(planes.data(), (int)planes.size(), n, slots, copy_src_dev, lens, stream);
}

}  // extern "C"

// ---- batched KV-cached decode (the precompute job: many short sequences against one pass over the weights) --------------
namespace {
// The launches of one decode step for the sequences in slots 0 .. B-1: ids from tok_buf / pos_buf, lengths and cache rows from ibuf, the final
// hidden states left in xn and the logits in logits_buf.  Captured into a graph by td_qwen2_decode_batch (nothing here may depend on a host value
// other than B and the engine's own pointers; max_len only sizes the generic attention entry's bookkeeping, the decode kernel reads kv_lens).
// vr_seqs > 0: the verify step of td_qwen2_verify_batch_slots.  The B rows are then the new tokens of vr_seqs sequences, up to vr_tmax each, sequence after
// sequence: ibuf holds row_off per ROW where it always does and the four per-SEQUENCE arrays of td_attn_verify_launch around it (first row | - | rows |
// keys visible to the first row | cache slot).  Everything but the attention is the step of B sequences; the rotary embedding and the cache write take
// their separate launch, so that every new k | v row is in the cache before the attention, which serves all rows of a sequence from one pass over it.
// lora: some row names an adapter (f->lora_rows is written).  The step then takes a launch list of its own: the low-rank add behind each of the four Linears,
// gate | up into the [B, 2 I] buffer with SiLU * up in a launch of its own (the fused GLU stream applies the activation before an update could be added), and on
// the wide path the RMSNorm out of the split-K reduction and into td_norm_rows_launch (the fused norm would read h before the update reaches it).
int decode_step(td_qwen2* f, int B, int max_len, bool want_logits, hipStream_t s, int vr_seqs = 0, int vr_tmax = 0, bool lora = false) {
  const int D = f->D, I = f->I, Hq = f->Hq, Hkv = f->Hkv;
  const int QW = Hq * 128, KVW = 2 * Hkv * 128;
  const int* kv_lens = f->ibuf;
  const int* row_off = f->ibuf + MAX_BATCH;
  const int* slot_ids = f->ibuf + 2 * MAX_BATCH;      // cache slot of each sequence of the step
  const bool verify = vr_seqs > 0;
  const bool fused_rope = f->fused_rope && !verify;
  // Cross-over between the weight-stream kernels and the tile kernels, measured on both decoder shapes (profiles/r4z_decode_crossover.log): the 2B
  // shape (hidden 1536) stays ahead on the stream through 64 sequences (2.68 vs 2.79 ms per step), the 7B shape (hidden 3584) is level at 24 and
  // 18 % ahead on the tiles at 64 (5.44 vs 6.63 ms).  TD_QWEN2_STREAM_BATCH (>= 16): A/B.
  static const int env_stream_batch = getenv("TD_QWEN2_STREAM_BATCH") ? atoi(getenv("TD_QWEN2_STREAM_BATCH")) : 0;
  const int stream_batch = env_stream_batch > 0 ? (env_stream_batch < 16 ? 16 : env_stream_batch) : (D >= 3072 ? 32 : STREAM_BATCH);
  // With the 8-bit (or 4-bit) stream on, a step of up to 64 sequences moves half (a quarter of) the bytes, so it stays on the stream kernels on both shapes
  // (tools/bench_qwen2_w8.py and tools/bench_qwen2_w4.py measure every batch bucket against the bf16 routing of the same handle)
  const bool wide = B > (f->w8_on ? STREAM_BATCH : stream_batch);
  // ... every bucket but one: two sequences measured 3 % SLOWER on the bytes than on bf16 W^ (1.503 vs 1.461 ms per step, profiles/qwen2_w8_bench.json),
  // so that step reads bf16 W^ -- the same model, no cost in numerics.  Measured on the 2B shape (hidden 1536) ONLY; the rule is drawn at the width
  // that already separates the two measured shapes (hidden < 3072), other narrow widths have not been timed.  The MXFP4 mode keeps the rule as it found it
  // (its own 2-sequence cell on the 2B shape was not timed); every other bucket measured faster on the nibbles than on bf16 W^ on both shapes
  const bool a8 = f->w_mode == TD_QWEN2_WEIGHTS_INT4 || !(B == 2 && D < 3072);      // (INT4 has a table of its own for every row count: int4_rows_routed)

  TD_TRY(td_embed_gather_launch(f->tok_buf, f->embed_w, f->h, B, D, f->cfg.vocab, s));
  TD_TRY(td_mrope_table_launch(f->pos_buf, B, f->cfg.mrope_section, f->cfg.rope_theta, 1, f->cosT, f->sinT, s));
  TdNormParams np;
  np.x = f->h; np.ldx = D; np.y = f->xn; np.ldy = D; np.rows = B; np.D = D; np.rms = 1; np.eps = f->cfg.rms_eps;
  for (int i = 0; i < f->cfg.num_layers; ++i) {
    const QLayer& l = f->layers[i];
    // (wide steps: the reduction launch of the Linear in front normalises the rows it finishes -- TdGemmParams::sk_norm_w -- so only layer 0 has a norm launch)
    if (!wide || lora || i == 0) {
      np.w = l.ln1_w;
      TD_TRY(td_norm_rows_launch(np, s));
    }
    {
      TdGemmParams g = linear(f->xn, D, l.qkv_w, l.qkv_b, f->q, QW, B, QW + KVW, D);
      g.C2 = f->kvtmp; g.ldc2 = KVW; g.n_split = QW;
      if (wide) { g.split_k = -1; g.sk_ws = f->sk_ws; g.sk_ws_bytes = SK_WS_BYTES; }      // (tile width and parts by the wide planner: n_split = Hq 128 fits its 64- / 128-column tiles)
      TD_TRY(run_linear(f, g, l.qkv_8, s, a8));
    }
    if (lora) TD_TRY(lora_add_qkv(f, i, f->kvtmp, B, s));
    // rotary embedding of the new q / k rows and the cache write ride inside the attention launch (TdAttnParams::dec_kv_new);
    // td_qwen2_set_fused_rope(f, 0): the separate launch (A/B and the bit-identity test)
    const bool kv8 = f->kv_mode == TD_QWEN2_KV_E4M3;
    if (!fused_rope) {
      if (kv8) hipLaunchKernelGGL(td_decode_rope_scatter_kernel<true>, dim3(B), dim3(256), 0, s, f->q, f->kvtmp, (bf16_t*)nullptr, l.kv8, l.kvs, row_off, f->cosT, f->sinT, Hq, Hkv);
      else hipLaunchKernelGGL(td_decode_rope_scatter_kernel<false>, dim3(B), dim3(256), 0, s, f->q, f->kvtmp, l.kv, (uint8_t*)nullptr, (float*)nullptr, row_off, f->cosT, f->sinT, Hq, Hkv);
    }
    TdAttnParams ap;
    if (fused_rope) { ap.dec_kv_new = f->kvtmp; ap.dec_cos = f->cosT; ap.dec_sin = f->sinT; ap.dec_row_off = row_off; }
    ap.Q = f->q; ap.ldq = QW; ap.q_bstride = QW; ap.ldkv = KVW;
    ap.kv_bstride = (long long)f->slot_len * KVW; ap.O = f->attn; ap.ldo = QW; ap.o_bstride = QW;
    ap.batch = B; ap.Sq = 1; ap.Skv = max_len; ap.Hq = Hq; ap.Hkv = Hkv; ap.scale = 0.08838834764831845f;
    ap.causal = 1; ap.causal_offset = max_len - 1; ap.kv_lens = kv_lens; ap.dec_slots = slot_ids;
    if (!kv8) {
      ap.K = l.kv; ap.V = l.kv + Hkv * 128;
    } else {      // the same launch, its descriptor carrying bytes + scales (ldkv / kv_bstride then count bytes)
      ap.K8 = l.kv8; ap.V8 = l.kv8 + Hkv * 128; ap.k_scale = l.kvs; ap.v_scale = l.kvs + Hkv; ap.lds = 2 * Hkv; ap.s_bstride = (long long)f->slot_len * 2 * Hkv;
    }
    if (verify) {
      ap.batch = vr_seqs; ap.kv_lens = nullptr; ap.dec_slots = nullptr;
      ap.vr_row0 = f->ibuf; ap.vr_rows = f->ibuf + 2 * MAX_BATCH; ap.vr_len0 = f->ibuf + 3 * MAX_BATCH; ap.vr_slot = f->ibuf + 4 * MAX_BATCH;
      TD_TRY(td_attn_verify_launch(ap, vr_tmax, s));
    } else {
      TD_TRY(td_attn_launch(ap, s));
    }
    {
      TdGemmParams g = linear(f->attn, QW, l.o_w, nullptr, f->h, D, B, D, QW, true);
      if (wide) {
        g.split_k = -1; g.sk_ws = f->sk_ws; g.sk_ws_bytes = SK_WS_BYTES;
        if (!lora) { g.sk_norm_w = l.ln2_w; g.sk_norm_out = f->xn; g.sk_norm_ld = D; g.sk_norm_eps = f->cfg.rms_eps; }
      }
      TD_TRY(run_linear(f, g, l.o_8, s, a8));
    }
    if (lora) TD_TRY(lora_add_o(f, i, B, s));
    if (!wide || lora) {
      np.w = l.ln2_w;
      TD_TRY(td_norm_rows_launch(np, s));
    }
    if (lora) {      // gate | up as one Linear, the add, then SiLU and product in a pass of their own (the prefill's rounding points)
      TdGemmParams g = linear(f->xn, D, l.gu_w, nullptr, f->gu, 2 * I, B, 2 * I, D);
      if (wide) { g.split_k = -1; g.sk_ws = f->sk_ws; g.sk_ws_bytes = SK_WS_BYTES; }
      if (wide) TD_TRY(td_gemm_launch(g, s));
      else TD_TRY(run_linear(f, g, l.gu_8, s, a8));
      TD_TRY(lora_add_gu(f, i, B, s));
      TD_TRY(td_silu_mul_launch(f->gu, f->act, B, I, s));
    } else if (!wide) {
      TdGemmParams g = linear(f->xn, D, l.gu_w, nullptr, f->act, I, B, I, D);
      g.glu_I = I;   // gate | up, SiLU and product in one pass
      TD_TRY(run_linear(f, g, l.gu_8, s, a8));
    } else {      // the prefill's form: gate | up as one Linear, SiLU and product in a pass of their own (the same rounding points)
      TdGemmParams g = linear(f->xn, D, l.gu_w, nullptr, f->gu, 2 * I, B, 2 * I, D);
      g.split_k = -1; g.sk_ws = f->sk_ws; g.sk_ws_bytes = SK_WS_BYTES;
      TD_TRY(td_gemm_launch(g, s));
      TD_TRY(td_silu_mul_launch(f->gu, f->act, B, I, s));
    }
    TdGemmParams d = linear(f->act, I, l.down_w, nullptr, f->h, D, B, D, I, true);
    if (wide) {
      d.split_k = -1; d.sk_ws = f->sk_ws; d.sk_ws_bytes = SK_WS_BYTES;
      if (!lora) {
        d.sk_norm_w = i + 1 < f->cfg.num_layers ? f->layers[i + 1].ln1_w : f->norm_w;      // the next layer's input norm, or model.norm
        d.sk_norm_out = f->xn; d.sk_norm_ld = D; d.sk_norm_eps = f->cfg.rms_eps;
      }
    }
    TD_TRY(run_linear(f, d, l.down_8, s, a8));
    if (lora) TD_TRY(lora_add_down(f, i, B, s));
  }
  if (!wide || lora) {
    np.w = f->norm_w; np.y = f->xn;
    TD_TRY(td_norm_rows_launch(np, s));
  }
  if (want_logits) TD_TRY(lm_head(f, f->xn, B, f->logits_buf, s, a8));
  TD_CHECK_LAUNCH();
  return TD_OK;
}
}  // namespace

extern "C" {

// One new token for each of the sequences in slots 0 .. B-1 (B <= 256): token_ids int32[B], position_ids int32[3,B] (device),
// cache_pos[b] = tokens already in slot b (HOST ints).  hidden_out bf16[B,hidden], logits bf16[B,vocab] (either may be NULL).
int td_qwen2_decode_batch(td_qwen2* f, int B, const int* token_ids, const int* position_ids, const int* cache_pos,
                          void* hidden_out, void* logits, void* stream) {
  return td_qwen2_decode_batch_slots(f, B, nullptr, token_ids, position_ids, cache_pos, hidden_out, logits, stream);
}

// ... for the sequences in cache slots slots[0 .. B-1] (HOST ints, distinct; NULL = 0 .. B-1): row b of the inputs and outputs belongs to slot slots[b].
// A finished sequence frees its slot with no cache rows moved, a new one is prefilled into any free slot (td_qwen2_prefill_packed_slots): the
// bookkeeping of continuous batching ([ext] vLLM's block tables, reduced to whole-sequence slots: 256 x 8192 rows fit the HBM outright).
int td_qwen2_decode_batch_slots(td_qwen2* f, int B, const int* slots, const int* token_ids, const int* position_ids, const int* cache_pos,
                                void* hidden_out, void* logits, void* stream) {
  TD_CHECK_ARG(f && token_ids && position_ids && cache_pos, "td_qwen2_decode_batch: null argument");
  TD_QWEN2_FRESH(f, "td_qwen2_decode_batch");
  TD_CHECK_ARG(B >= 1 && B <= MAX_BATCH && B <= f->n_slots && B <= f->ws_rows, "td_qwen2_decode_batch: batch %d exceeds min(%d, %d slots, %d workspace rows)", B, MAX_BATCH, f->n_slots, f->ws_rows);
  hipStream_t s = (hipStream_t)stream;
  const int D = f->D;
  IntPack ip;
  int max_len = 0;
  if (slots) TD_TRY(check_distinct_slots("td_qwen2_decode_batch", "row", slots, B));
  for (int b = 0; b < B; ++b) {
    const int slot = slots ? slots[b] : b;
    TD_CHECK_ARG(slot >= 0 && slot < f->n_slots, "td_qwen2_decode_batch: sequence %d names cache slot %d of %d", b, slot, f->n_slots);
    TD_CHECK_ARG(cache_pos[b] >= 0 && cache_pos[b] < f->slot_len, "td_qwen2_decode_batch: sequence %d is full (%d of %d)", b, cache_pos[b], f->slot_len);
    ip.v[b] = cache_pos[b] + 1;                                         // keys visible to the new token
    ip.v[MAX_BATCH + b] = slot * f->slot_len + cache_pos[b];            // its cache row (index; the kernels scale it by the row width)
    ip.v[2 * MAX_BATCH + b] = slot;
    max_len = cache_pos[b] + 1 > max_len ? cache_pos[b] + 1 : max_len;
  }
  hipLaunchKernelGGL(td_set_ints_kernel, dim3(1), dim3(3 * MAX_BATCH), 0, s, f->ibuf, ip, 3 * MAX_BATCH);
  TD_CHECK_LAUNCH();
  bool lora = false;      // the rows' adapters from the slot map: device data, so a captured LoRA step replays under a changed assignment
  if (f->lora_max > 0) {
    int rc;
    f->lora_rows_host.resize((size_t)B);
    for (int b = 0; b < B; ++b) f->lora_rows_host[(size_t)b] = f->slot_adapter(slots ? slots[b] : b);
    lora = lora_upload_rows(f, B, s, &rc);
    TD_TRY(rc);
  }
  // the step reads its ids from fixed buffers and leaves its outputs in fixed buffers (the captured form needs stable addresses)
  TD_CHECK_HIP(hipMemcpyAsync(f->tok_buf, token_ids, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(f->pos_buf, position_ids, (size_t)3 * B * 4, hipMemcpyDeviceToDevice, s));
  const bool want_logits = logits != nullptr;
  const int key = 2 * B + (want_logits ? 1 : 0) + (lora ? 1 << 20 : 0);      // (a LoRA step is another launch list)
  static const bool no_graph = getenv("TD_QWEN2_NO_GRAPH") != nullptr;
  auto it = f->step_graphs.find(key);
  if (it != f->step_graphs.end()) {
    TD_CHECK_HIP(hipGraphLaunch(it->second, s));
  } else if (no_graph || !f->graphs_ok || f->step_calls[key]++ == 0) {
    TD_TRY(decode_step(f, B, max_len, want_logits, s, 0, 0, lora));
  } else {
    // capture on the engine's own stream (the caller's may be the legacy default stream, which cannot capture), after everything the caller
    // queued so far: nothing runs during a capture, but the eager fallback below must see the ids copied above
    if (!f->capture_stream) TD_CHECK_HIP(hipStreamCreateWithFlags(&f->capture_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool ok = hipStreamBeginCapture(f->capture_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
      const int rc = decode_step(f, B, max_len, want_logits, f->capture_stream, 0, 0, lora);
      ok = hipStreamEndCapture(f->capture_stream, &graph) == hipSuccess && rc == TD_OK && graph != nullptr;
    }
    if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
    if (getenv("TD_QWEN2_GRAPH_DEBUG")) fprintf(stderr, "td_qwen2_decode_batch: step graph for B=%d logits=%d %s\n", B, (int)want_logits, ok ? "captured" : "NOT captured (eager from now on)");
    if (ok) {
      f->step_graphs[key] = exec;
      TD_CHECK_HIP(hipGraphLaunch(exec, s));
    } else {
      (void)hipGetLastError();
      f->graphs_ok = false;      // this runtime cannot capture the step: stay on the eager path for good
      TD_TRY(decode_step(f, B, max_len, want_logits, s, 0, 0, lora));
    }
  }
  if (hidden_out) TD_CHECK_HIP(hipMemcpyAsync(hidden_out, f->xn, (size_t)B * D * 2, hipMemcpyDeviceToDevice, s));
  if (logits) TD_CHECK_HIP(hipMemcpyAsync(logits, f->logits_buf, (size_t)B * f->cfg.vocab * 2, hipMemcpyDeviceToDevice, s));
  return TD_OK;
}

// The verify step of speculative decoding (include/thinkdiff_hip.h): sequence b feeds n_new[b] tokens at cache rows cache_pos[b] .., R = sum n_new rows in
// all.  decode_step over R rows with the multi-row attention; eager.  Every n_new == 1: the plain step itself.
int td_qwen2_verify_batch_slots(td_qwen2* f, int B, const int* slots, const int* n_new, const int* token_ids, const int* position_ids, const int* cache_pos,
                                void* hidden_out, void* logits, void* stream) {
  TD_CHECK_ARG(f && n_new && token_ids && position_ids && cache_pos, "td_qwen2_verify_batch: null argument");
  TD_QWEN2_FRESH(f, "td_qwen2_verify_batch");
  TD_CHECK_ARG(B >= 1 && B <= MAX_BATCH && B <= f->n_slots && B <= f->ws_rows, "td_qwen2_verify_batch: batch %d exceeds min(%d, %d slots, %d workspace rows)", B, MAX_BATCH, f->n_slots, f->ws_rows);
  if (slots) TD_TRY(check_distinct_slots("td_qwen2_verify_batch", "sequence", slots, B));
  IntPack rows_pack, seq_pack;      // ibuf [0, 3 MAX_BATCH): first row per sequence | cache row per ROW | rows per sequence; [3 MAX_BATCH, 5 MAX_BATCH): len0 | slot
  int R = 0, max_len = 0, t_max = 1;
  for (int b = 0; b < B; ++b) {
    const int slot = slots ? slots[b] : b;
    TD_CHECK_ARG(slot >= 0 && slot < f->n_slots, "td_qwen2_verify_batch: sequence %d names cache slot %d of %d", b, slot, f->n_slots);
    TD_CHECK_ARG(n_new[b] >= 1 && n_new[b] <= TD_MAX_VERIFY_ROWS, "td_qwen2_verify_batch: n_new[%d]=%d outside 1..%d", b, n_new[b], TD_MAX_VERIFY_ROWS);
    TD_CHECK_ARG(cache_pos[b] >= 0 && cache_pos[b] + n_new[b] <= f->slot_len, "td_qwen2_verify_batch: sequence %d: cache_pos %d + n_new %d exceeds the slot capacity %d", b,
                 cache_pos[b], n_new[b], f->slot_len);
    TD_CHECK_ARG(R + n_new[b] <= MAX_BATCH && R + n_new[b] <= f->ws_rows, "td_qwen2_verify_batch: R=%d rows exceed min(%d, %d workspace rows)", R + n_new[b], MAX_BATCH, f->ws_rows);
    rows_pack.v[b] = R;
    rows_pack.v[2 * MAX_BATCH + b] = n_new[b];
    seq_pack.v[b] = cache_pos[b] + 1;
    seq_pack.v[MAX_BATCH + b] = slot;
    for (int j = 0; j < n_new[b]; ++j) rows_pack.v[MAX_BATCH + R + j] = slot * f->slot_len + cache_pos[b] + j;
    R += n_new[b];
    t_max = n_new[b] > t_max ? n_new[b] : t_max;
    max_len = cache_pos[b] + n_new[b] > max_len ? cache_pos[b] + n_new[b] : max_len;
  }
  if (t_max == 1) return td_qwen2_decode_batch_slots(f, B, slots, token_ids, position_ids, cache_pos, hidden_out, logits, stream);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(td_set_ints_kernel, dim3(1), dim3(3 * MAX_BATCH), 0, s, f->ibuf, rows_pack, 3 * MAX_BATCH);
  hipLaunchKernelGGL(td_set_ints_kernel, dim3(1), dim3(3 * MAX_BATCH), 0, s, f->ibuf + 3 * MAX_BATCH, seq_pack, 2 * MAX_BATCH);
  TD_CHECK_LAUNCH();
  TD_CHECK_HIP(hipMemcpyAsync(f->tok_buf, token_ids, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
  // (pos_buf is [3, R] here: the table launch reads stream k of row r at k R + r)
  TD_CHECK_HIP(hipMemcpyAsync(f->pos_buf, position_ids, (size_t)3 * R * 4, hipMemcpyDeviceToDevice, s));
  bool lora = false;      // a sequence's adapter on all of its rows
  if (f->lora_max > 0) {
    int rc;
    f->lora_rows_host.resize((size_t)R);
    for (int b = 0, r = 0; b < B; ++b)
      for (int j = 0; j < n_new[b]; ++j) f->lora_rows_host[(size_t)r++] = f->slot_adapter(slots ? slots[b] : b);
    lora = lora_upload_rows(f, R, s, &rc);
    TD_TRY(rc);
  }
  TD_TRY(decode_step(f, R, max_len, logits != nullptr, s, B, t_max, lora));
  if (hidden_out) TD_CHECK_HIP(hipMemcpyAsync(hidden_out, f->xn, (size_t)R * f->D * 2, hipMemcpyDeviceToDevice, s));
  if (logits) TD_CHECK_HIP(hipMemcpyAsync(logits, f->logits_buf, (size_t)R * f->cfg.vocab * 2, hipMemcpyDeviceToDevice, s));
  return TD_OK;
}

// Prefill of B sequences in one pass: every sequence is right-padded to L tokens (row b * L + t; causal attention keeps the
// padding from influencing real tokens), sequence b goes to cache slot b.  inputs_embeds bf16[B*L, hidden] or token_ids
// int32[B*L]; position_ids int32[3, B*L]; lens[b] = real tokens of sequence b (HOST ints).  hidden_out bf16[B*L, hidden]
// (rows past lens[b] are meaningless), logits_last bf16[B, vocab] of each sequence's last real token (either may be NULL).
int td_qwen2_prefill_batch(td_qwen2* f, int B, int L, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                           const int* lens, void* hidden_out, void* logits_last, void* stream) {
  return td_qwen2_prefill_batch_at(f, 0, B, L, token_ids, inputs_embeds, position_ids, lens, hidden_out, logits_last, stream);
}

// ... into cache slots slot0 .. slot0 + B - 1 (a request batch larger than the activation workspace is prefilled in several calls)
int td_qwen2_prefill_batch_at(td_qwen2* f, int slot0, int B, int L, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                              const int* lens, void* hidden_out, void* logits_last, void* stream) {
  TD_CHECK_ARG(f && position_ids && lens && (token_ids || inputs_embeds), "td_qwen2_prefill_batch: null argument");
  TD_QWEN2_FRESH(f, "td_qwen2_prefill_batch");
  TD_CHECK_ARG(slot0 >= 0 && B >= 1 && B <= MAX_BATCH && slot0 + B <= f->n_slots && L >= 1 && L <= f->slot_len && (long long)B * L <= f->ws_rows,
               "td_qwen2_prefill_batch: slots [%d, %d) x L=%d exceed the handle (slots %d x %d tokens, workspace %d rows)", slot0, slot0 + B, L, f->n_slots, f->slot_len, f->ws_rows);
  for (int b = 0; b < B; ++b) TD_CHECK_ARG(lens[b] >= 1 && lens[b] <= L, "td_qwen2_prefill_batch: sequence %d has %d of %d tokens", b, lens[b], L);
  hipStream_t s = (hipStream_t)stream;
  const int D = f->D, QW = f->Hq * 128;
  const long long KVW = 2 * f->Hkv * 128, kv0 = (long long)slot0 * f->slot_len * KVW;      // first slot of this call
  PrefillForm form;
  form.n = B * L;
  form.attn = prefill_attn(f, B, L, L, 0);
  form.attn.q_bstride = form.attn.o_bstride = (long long)L * QW;
  if (f->kv_mode == TD_QWEN2_KV_E4M3) {      // the attention reads the rounded rows in kvtmp; the quantising scatter takes the cache row of every row
    f->row_map_host.resize((size_t)B * L);
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < L; ++t) f->row_map_host[(size_t)b * L + t] = (slot0 + b) * f->slot_len + t;
    TD_CHECK_HIP(hipMemcpyAsync(f->row_map, f->row_map_host.data(), (size_t)B * L * 4, hipMemcpyHostToDevice, s));
    form.to_rows = f->row_map;
    form.attn.kv_bstride = L * KVW;
  } else {
    form.to_slots = kv0; form.slots_L = L;
    form.attn.kv_bstride = f->slot_len * KVW;
    form.attn_kv = KvRows{kv0};
  }
  if (f->lora_max > 0) {
    int rc;
    f->lora_rows_host.resize((size_t)B * L);
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < L; ++t) f->lora_rows_host[(size_t)b * L + t] = f->slot_adapter(slot0 + b);
    form.lora = lora_upload_rows(f, B * L, s, &rc);
    TD_TRY(rc);
  }
  TD_TRY(prefill_pass(f, form, token_ids, inputs_embeds, position_ids, hidden_out, s));
  if (logits_last) {
    for (int b = 0; b < B; ++b)
      TD_CHECK_HIP(hipMemcpyAsync(f->lastrows + (size_t)b * D, f->xn + ((size_t)b * L + lens[b] - 1) * D, (size_t)D * 2, hipMemcpyDeviceToDevice, s));
    TD_TRY(lm_head(f, f->lastrows, B, logits_last, s));
  }
  TD_CHECK_LAUNCH();
  return TD_OK;
}

// Packed prefill: the B prompts lie back to back (row offsets = the running sum of lens; no padding rows), sequence b goes to cache slot slot0 + b.
// What vLLM's scheduler does with the reference's request batches (max_num_batched_tokens rows per pass); against the padded form it saves the
// rows between each prompt and the longest.  total = sum(lens) rows: inputs_embeds bf16[total, hidden] or token_ids int32[total]; position_ids
// int32[3, total]; hidden_out bf16[total, hidden]; logits_last bf16[B, vocab] of each prompt's last token (either output may be NULL).
int td_qwen2_prefill_packed(td_qwen2* f, int slot0, int B, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                            const int* lens, void* hidden_out, void* logits_last, void* stream) {
  TD_CHECK_ARG(slot0 >= 0 && B >= 1 && B <= MAX_BATCH, "td_qwen2_prefill_packed: bad slot range");
  int slots[MAX_BATCH];
  for (int b = 0; b < B; ++b) slots[b] = slot0 + b;
  return td_qwen2_prefill_packed_slots(f, B, slots, token_ids, inputs_embeds, position_ids, lens, hidden_out, logits_last, stream);
}

// ... sequence b into cache slot slots[b] (HOST ints, distinct, any order): the free slots of a running batch
int td_qwen2_prefill_packed_slots(td_qwen2* f, int B, const int* slots, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                                  const int* lens, void* hidden_out, void* logits_last, void* stream) {
  TD_CHECK_ARG(f && slots && position_ids && lens && (token_ids || inputs_embeds), "td_qwen2_prefill_packed: null argument");
  TD_QWEN2_FRESH(f, "td_qwen2_prefill_packed");
  TD_CHECK_ARG(B >= 1 && B <= MAX_BATCH, "td_qwen2_prefill_packed: %d sequences (1 .. %d)", B, MAX_BATCH);
  for (int b = 0; b < B; ++b) TD_CHECK_ARG(slots[b] >= 0 && slots[b] < f->n_slots, "td_qwen2_prefill_packed: sequence %d names cache slot %d of %d", b, slots[b], f->n_slots);
  TD_TRY(check_distinct_slots("td_qwen2_prefill_packed", "sequence", slots, B));
  long long total = 0;
  int L = 0;
  for (int b = 0; b < B; ++b) {
    TD_CHECK_ARG(lens[b] >= 1 && lens[b] <= f->slot_len, "td_qwen2_prefill_packed: sequence %d has %d tokens (slot capacity %d)", b, lens[b], f->slot_len);
    total += lens[b];
    L = lens[b] > L ? lens[b] : L;
  }
  TD_CHECK_ARG(total <= f->ws_rows, "td_qwen2_prefill_packed: %lld packed rows exceed the %d workspace rows", total, f->ws_rows);
  hipStream_t s = (hipStream_t)stream;
  const int D = f->D, n = (int)total;
  // segment starts (device, for the attention and the last-row gather) and the cache row of every packed row
  IntPack ip;
  int* seg_starts = f->ibuf + 3 * MAX_BATCH;      // [B + 1] behind the decode step's lengths, rows and slots
  static_assert(MAX_BATCH + 1 <= 3 * MAX_BATCH, "seg_starts fit one IntPack");
  f->row_map_host.resize((size_t)n);
  int r = 0;
  for (int b = 0; b < B; ++b) {
    ip.v[b] = r;
    for (int t = 0; t < lens[b]; ++t) f->row_map_host[(size_t)r + t] = slots[b] * f->slot_len + t;
    r += lens[b];
  }
  ip.v[B] = r;
  hipLaunchKernelGGL(td_set_ints_kernel, dim3(1), dim3(3 * MAX_BATCH), 0, s, seg_starts, ip, B + 1);
  TD_CHECK_LAUNCH();
  TD_CHECK_HIP(hipMemcpyAsync(f->row_map, f->row_map_host.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  PrefillForm form;
  form.n = n;
  form.to_rows = f->row_map;
  form.attn = prefill_attn(f, B, L, L, 0);      // causal attention inside each packed prompt, straight from the projection rows (a prefill starts at position 0)
  form.attn.seg_starts = seg_starts;
  if (f->lora_max > 0) {
    int rc;
    f->lora_rows_host.resize((size_t)n);
    for (int b = 0, q = 0; b < B; ++b)
      for (int t = 0; t < lens[b]; ++t) f->lora_rows_host[(size_t)q++] = f->slot_adapter(slots[b]);
    form.lora = lora_upload_rows(f, n, s, &rc);
    TD_TRY(rc);
  }
  TD_TRY(prefill_pass(f, form, token_ids, inputs_embeds, position_ids, hidden_out, s));
  if (logits_last) {
    hipLaunchKernelGGL(td_gather_last_rows_kernel, dim3((D / 8 + 255) / 256, B), dim3(256), 0, s, f->xn, f->lastrows, seg_starts, D);
    TD_TRY(lm_head(f, f->lastrows, B, logits_last, s));
  }
  TD_CHECK_LAUNCH();
  return TD_OK;
}

// Packed prefill behind cached prefixes (automatic prefix caching): sequence b feeds lens[b] >= 1 NEW rows, which go to cache rows [prefix_lens[b],
// prefix_lens[b] + lens[b]) of slot slots[b]; the caller vouches that the first prefix_lens[b] rows of that slot are valid.  The packed operands and outputs
// cover the new rows only, laid out as in td_qwen2_prefill_packed_slots, which every prefix_lens[b] == 0 delegates to.  bf16 cache: the new k | v rows are
// scattered to their cache rows in front of the attention, which reads K / V straight from the layer's cache, every query segment over its own slot's rows
// [0, prefix + len) (TdAttnParams::kv_seg_row0 / kv_seg_lens).  e4m3 cache: staged -- the new rows are quantised into the cache, rows [0, prefix + len) of every
// sequence are dequantised into f->kvstage, packed per segment, by ONE row-mapped launch per layer, and the attention runs over that buffer.
int td_qwen2_prefill_packed_prefix_slots(td_qwen2* f, int B, const int* slots, const int* token_ids, const void* inputs_embeds, const int* position_ids,
                                         const int* lens, const int* prefix_lens, void* hidden_out, void* logits_last, void* stream) {
  TD_CHECK_ARG(f && slots && position_ids && lens && prefix_lens && (token_ids || inputs_embeds), "td_qwen2_prefill_packed_prefix: null argument");
  TD_QWEN2_FRESH(f, "td_qwen2_prefill_packed_prefix");
  TD_CHECK_ARG(B >= 1 && B <= MAX_BATCH, "td_qwen2_prefill_packed_prefix: %d sequences (1 .. %d)", B, MAX_BATCH);
  for (int b = 0; b < B; ++b) TD_CHECK_ARG(slots[b] >= 0 && slots[b] < f->n_slots, "td_qwen2_prefill_packed_prefix: sequence %d names cache slot %d of %d", b, slots[b], f->n_slots);
  TD_TRY(check_distinct_slots("td_qwen2_prefill_packed_prefix", "sequence", slots, B));
  long long total = 0, staged = 0;
  int L = 0, Lkv = 0;
  bool any_prefix = false;
  for (int b = 0; b < B; ++b) {
    TD_CHECK_ARG(lens[b] >= 1, "td_qwen2_prefill_packed_prefix: sequence %d feeds lens=%d rows (at least 1)", b, lens[b]);
    TD_CHECK_ARG(prefix_lens[b] >= 0, "td_qwen2_prefill_packed_prefix: sequence %d has prefix_lens=%d (at least 0)", b, prefix_lens[b]);
    TD_CHECK_ARG((long long)prefix_lens[b] + lens[b] <= f->slot_len, "td_qwen2_prefill_packed_prefix: sequence %d: prefix %d + %d new rows exceed the slot capacity %d", b,
                 prefix_lens[b], lens[b], f->slot_len);
    total += lens[b];
    staged += prefix_lens[b] + lens[b];
    L = lens[b] > L ? lens[b] : L;
    Lkv = prefix_lens[b] + lens[b] > Lkv ? prefix_lens[b] + lens[b] : Lkv;
    any_prefix = any_prefix || prefix_lens[b] > 0;
  }
  TD_CHECK_ARG(total <= f->ws_rows, "td_qwen2_prefill_packed_prefix: %lld packed rows exceed the %d workspace rows", total, f->ws_rows);
  if (!any_prefix) return td_qwen2_prefill_packed_slots(f, B, slots, token_ids, inputs_embeds, position_ids, lens, hidden_out, logits_last, stream);
  const bool kv8 = f->kv_mode == TD_QWEN2_KV_E4M3;
  if (kv8) TD_CHECK_ARG(staged <= f->ws_rows, "td_qwen2_prefill_packed_prefix: the e4m3 cache stages prefix + new rows: %lld staged rows exceed the %d workspace rows", staged, f->ws_rows);
  hipStream_t s = (hipStream_t)stream;
  const int D = f->D, n = (int)total, KVW = 2 * f->Hkv * 128;
  if (kv8 && !f->kvstage) {      // the staging buffer and its row map, at the first pass that needs them
    const size_t rows_bytes = ((size_t)f->ws_rows * KVW * 2 + 255) & ~(size_t)255;
    TD_CHECK_HIP(hipMalloc((void**)&f->kvstage, rows_bytes + (size_t)f->ws_rows * 4));
    f->stage_map = (int*)((char*)f->kvstage + rows_bytes);
  }
  // device ints: seg_starts [B + 1] where the packed prefill keeps them, the first key row and the key count of every segment behind the verify step's arrays;
  // the cache row of every packed new row, and (e4m3) of every staged row
  IntPack ip, kp;
  int* seg_starts = f->ibuf + 3 * MAX_BATCH;
  int* kv_row0 = f->ibuf + 5 * MAX_BATCH;
  int* kv_lens = f->ibuf + 6 * MAX_BATCH;
  f->row_map_host.resize((size_t)n + (kv8 ? (size_t)staged : 0));
  int r = 0, sr = 0;
  for (int b = 0; b < B; ++b) {
    const int row0 = slots[b] * f->slot_len, klen = prefix_lens[b] + lens[b];
    ip.v[b] = r;
    kp.v[b] = kv8 ? sr : row0;
    kp.v[MAX_BATCH + b] = klen;
    for (int t = 0; t < lens[b]; ++t) f->row_map_host[(size_t)r + t] = row0 + prefix_lens[b] + t;
    if (kv8)
      for (int t = 0; t < klen; ++t) f->row_map_host[(size_t)n + sr + t] = row0 + t;
    r += lens[b];
    sr += klen;
  }
  ip.v[B] = r;
  hipLaunchKernelGGL(td_set_ints_kernel, dim3(1), dim3(3 * MAX_BATCH), 0, s, seg_starts, ip, B + 1);
  hipLaunchKernelGGL(td_set_ints_kernel, dim3(1), dim3(3 * MAX_BATCH), 0, s, kv_row0, kp, 2 * MAX_BATCH);
  TD_CHECK_LAUNCH();
  TD_CHECK_HIP(hipMemcpyAsync(f->row_map, f->row_map_host.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  if (kv8) TD_CHECK_HIP(hipMemcpyAsync(f->stage_map, f->row_map_host.data() + n, (size_t)staged * 4, hipMemcpyHostToDevice, s));
  PrefillForm form;
  form.n = n;
  form.to_rows = f->row_map;
  form.attn = prefill_attn(f, B, L, Lkv, 0);      // (the segments' causal offsets are prefix_lens: the kernel takes them from kv_seg_lens)
  form.attn.seg_starts = seg_starts;
  form.attn.kv_seg_row0 = kv_row0;
  form.attn.kv_seg_lens = kv_lens;
  if (kv8) { form.q8_stage_rows = f->stage_map; form.q8_stage_n = (int)staged; }
  else form.attn_kv = KvRows{0};                  // K / V = the layer's cache, seen as rows
  if (f->lora_max > 0) {
    int rc;
    f->lora_rows_host.resize((size_t)n);
    for (int b = 0, q = 0; b < B; ++b)
      for (int t = 0; t < lens[b]; ++t) f->lora_rows_host[(size_t)q++] = f->slot_adapter(slots[b]);
    form.lora = lora_upload_rows(f, n, s, &rc);
    TD_TRY(rc);
  }
  TD_TRY(prefill_pass(f, form, token_ids, inputs_embeds, position_ids, hidden_out, s));
  if (logits_last) {
    hipLaunchKernelGGL(td_gather_last_rows_kernel, dim3((D / 8 + 255) / 256, B), dim3(256), 0, s, f->xn, f->lastrows, seg_starts, D);
    TD_TRY(lm_head(f, f->lastrows, B, logits_last, s));
  }
  TD_CHECK_LAUNCH();
  return TD_OK;
}

// ---- per-request LoRA: the adapter pool, the slot map and what the passes above read ------------------------------------------------------------------------

int td_qwen2_lora_enable(td_qwen2* f, int max_loras, int max_rank) {
  TD_CHECK_ARG(f, "td_qwen2_lora_enable: null handle");
  TD_CHECK_ARG(max_loras >= 1 && max_loras <= TD_LORA_MAX_ADAPTERS, "td_qwen2_lora_enable: max_loras=%d outside 1..%d", max_loras, TD_LORA_MAX_ADAPTERS);
  TD_CHECK_ARG(max_rank >= 1 && max_rank <= TD_LORA_ROWS_MAX_RANK, "td_qwen2_lora_enable: max_rank=%d outside 1..%d", max_rank, TD_LORA_ROWS_MAX_RANK);
  TD_CHECK_ARG(f->lora_max == 0, "td_qwen2_lora_enable: LoRA is enabled on this handle already (max_loras=%d, max_rank=%d)", f->lora_max, f->lora_max_rank);
  const int D = f->D, I = f->I, QW = f->Hq * 128, HW = f->Hkv * 128;
  const int N[7] = {QW, HW, HW, D, I, I, D}, K[7] = {D, D, D, QW, D, D, I};
  auto pad = [](int64_t b) { return (b + 255) & ~int64_t(255); };
  int64_t block = 0, place[7];
  for (int m = 0; m < 7; ++m) {
    TD_CHECK_ARG(N[m] % 16 == 0 && K[m] % 64 == 0, "td_qwen2_lora_enable: the low-rank kernels need every Linear's N=%d %% 16 == 0 and K=%d %% 64 == 0", N[m], K[m]);
    place[m] = block;
    block += pad((int64_t)td_lora_rows_packed_bytes(max_rank, N[m], K[m]));
  }
  const int64_t pool = block * max_loras * (int64_t)f->layers.size();
  size_t ws = 0;
  const int wsK[4] = {D, QW, D, I}, wsS[4] = {3, 1, 2, 1};
  for (int i = 0; i < 4; ++i) ws = std::max(ws, td_lora_rows_workspace_bytes(f->ws_rows, wsK[i], wsS[i], max_rank));
  const int64_t rows_bytes = pad((int64_t)f->ws_rows * 4);
  hipError_t e = hipMalloc((void**)&f->lora_arena, (size_t)(pool + rows_bytes + pad((int64_t)ws)));
  if (e != hipSuccess) {
    f->lora_arena = nullptr;
    td_set_error("td_qwen2_lora_enable: hipMalloc of %.2f GiB for %d adapters of rank %d failed: %s", (pool + rows_bytes + ws) / double(1 << 30), max_loras, max_rank,
                 hipGetErrorString(e));
    return TD_ERR_HIP;
  }
  f->lora_max = max_loras; f->lora_max_rank = max_rank;
  f->lora_pool_bytes = pool; f->lora_block = block;
  for (int m = 0; m < 7; ++m) f->lora_place[m] = place[m];
  f->lora_rows = (int*)(f->lora_arena + pool);
  f->lora_ws = f->lora_arena + pool + rows_bytes;
  f->lora_ws_bytes = ws;
  f->lora_have.assign((size_t)max_loras * f->layers.size() * 7, 0);
  f->lora_rank.assign((size_t)TD_LORA_MAX_ADAPTERS, 0);
  f->lora_count.assign((size_t)TD_LORA_MAX_ADAPTERS, 0);
  f->lora_scale.assign((size_t)TD_LORA_MAX_ADAPTERS, 0.f);
  f->slot_lora.clear();
  drop_step_graphs(f);
  return TD_OK;
}

int td_qwen2_lora_load(td_qwen2* f, int index, const char* module, const void* A, const void* B, int rank, float scale, void* stream) {
  TD_CHECK_ARG(f && module && A && B, "td_qwen2_lora_load: the handle, module, A and B are required");
  TD_CHECK_ARG(f->lora_max > 0, "td_qwen2_lora_load: LoRA is not enabled on this handle (td_qwen2_lora_enable first)");
  TD_CHECK_ARG(index >= 0 && index < f->lora_max, "td_qwen2_lora_load: index=%d outside the %d adapters of the pool", index, f->lora_max);
  TD_CHECK_ARG(rank >= 1 && rank <= f->lora_max_rank, "td_qwen2_lora_load: rank=%d outside 1..%d (max_rank of td_qwen2_lora_enable)", rank, f->lora_max_rank);
  TD_CHECK_ARG(scale == scale && scale - scale == 0.f, "td_qwen2_lora_load: scale is not finite");
  int layer = -1, used = 0;
  char sub[16] = {0}, name[16] = {0};
  const bool parsed = sscanf(module, "model.layers.%d.%15[a-z_].%15[a-z_]%n", &layer, sub, name, &used) == 3 && module[used] == 0;
  static const char* const names[7] = {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"};
  int m = -1;
  if (parsed)
    for (int i = 0; i < 7; ++i)
      if ((std::string(sub) + "." + name) == names[i]) m = i;
  TD_CHECK_ARG(m >= 0 && layer >= 0 && layer < (int)f->layers.size(),
               "td_qwen2_lora_load: module '%s' is not one of the 7 Linears of a decoder layer (model.layers.N.self_attn.{q,k,v,o}_proj, model.layers.N.mlp.{gate,up,down}_proj, "
               "N < %d)", module, (int)f->layers.size());
  TD_CHECK_ARG(f->lora_count[(size_t)index] == 0 || (f->lora_rank[(size_t)index] == rank && f->lora_scale[(size_t)index] == scale),
               "td_qwen2_lora_load: adapter %d holds pairs of rank=%d, scale=%g; '%s' comes with rank=%d, scale=%g (one rank and scale per adapter: rank_pattern / "
               "alpha_pattern are not served)", index, f->lora_rank[(size_t)index], f->lora_scale[(size_t)index], module, rank, scale);
  const int D = f->D, I = f->I, QW = f->Hq * 128, HW = f->Hkv * 128;
  const int N[7] = {QW, HW, HW, D, I, I, D}, K[7] = {D, D, D, QW, D, D, I};
  drop_step_graphs(f);      // the captured LoRA steps carry which pairs exist, their ranks and scales
  char* dst = f->lora_arena + ((size_t)index * f->layers.size() + layer) * f->lora_block + f->lora_place[m];
  TD_TRY(td_lora_rows_pack_bf16(A, B, rank, N[m], K[m], dst, stream));
  char& have = f->lora_have[((size_t)index * f->layers.size() + layer) * 7 + m];
  if (!have) { have = 1; ++f->lora_count[(size_t)index]; }
  f->lora_rank[(size_t)index] = rank;
  f->lora_scale[(size_t)index] = scale;
  return TD_OK;
}

int td_qwen2_lora_remove(td_qwen2* f, int index) {
  TD_CHECK_ARG(f, "td_qwen2_lora_remove: null handle");
  TD_CHECK_ARG(f->lora_max > 0, "td_qwen2_lora_remove: LoRA is not enabled on this handle (td_qwen2_lora_enable first)");
  TD_CHECK_ARG(index >= 0 && index < f->lora_max, "td_qwen2_lora_remove: index=%d outside the %d adapters of the pool", index, f->lora_max);
  const size_t per = f->layers.size() * 7;
  std::fill(f->lora_have.begin() + (size_t)index * per, f->lora_have.begin() + (size_t)(index + 1) * per, 0);
  f->lora_count[(size_t)index] = 0;
  f->lora_rank[(size_t)index] = 0;
  f->lora_scale[(size_t)index] = 0.f;
  for (int& a : f->slot_lora)
    if (a == index) a = -1;      // no slot keeps naming a place that another adapter may take
  drop_step_graphs(f);
  return TD_OK;
}

int td_qwen2_lora_set_slot(td_qwen2* f, int slot, int index) {
  TD_CHECK_ARG(f, "td_qwen2_lora_set_slot: null handle");
  TD_CHECK_ARG(slot >= 0 && slot < f->n_slots, "td_qwen2_lora_set_slot: slot %d outside the %d configured sequences", slot, f->n_slots);
  TD_CHECK_ARG(index == -1 || f->lora_max > 0, "td_qwen2_lora_set_slot: LoRA is not enabled on this handle (td_qwen2_lora_enable first)");
  TD_CHECK_ARG(index >= -1 && index < f->lora_max, "td_qwen2_lora_set_slot: index=%d outside -1 (no adapter) .. %d", index, f->lora_max - 1);
  if (index < 0 && slot >= (int)f->slot_lora.size()) return TD_OK;
  if ((int)f->slot_lora.size() <= slot) f->slot_lora.resize((size_t)slot + 1, -1);
  f->slot_lora[(size_t)slot] = index;
  return TD_OK;
}

int td_qwen2_lora_info(const td_qwen2* f, int* max_loras, int* resident, int64_t* bytes, int64_t* launches) {
  TD_CHECK_ARG(f, "td_qwen2_lora_info: null handle");
  int n = 0;
  for (int c : f->lora_count) n += c > 0 ? 1 : 0;
  if (max_loras) *max_loras = f->lora_max;
  if (resident) *resident = n;
  if (bytes) *bytes = f->lora_max > 0 ? f->lora_pool_bytes + (int64_t)f->lora_ws_bytes + (int64_t)f->ws_rows * 4 : 0;
  if (launches) *launches = f->lora_launches;
  return TD_OK;
}

}  // extern "C"
