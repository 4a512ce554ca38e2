// FLUX.1 MMDiT denoise engine: host-side C++ that owns the fused weight arena + activation
// workspace in HBM and issues the per-step kernel sequence (one stream, no host sync, no
// allocation after creation).
//
// Replaces, for the ThinkDiff drivers' `diffusion_pipe(prompt_embeds=..., pooled_prompt_embeds=...)`
// call (reference scripts/test/test_blip_vision_t5_decoder_flux_text.py:234-242,
// scripts/test/test_mllama_t5_decoder_flux.py:182-192):
//   [ext diffusers 0.31.0] FluxTransformer2DModel.forward, FluxPosEmbed,
//   CombinedTimestepGuidanceTextProjEmbeddings, AdaLayerNormZero(/Single/Continuous),
//   FluxAttnProcessor2_0, FlowMatchEulerDiscreteScheduler.step.
//
// MI355X-first layout decisions
//  * text and image streams live in ONE token-major buffer h[S = T + S_img, D] (text rows first,
//    the order diffusers concatenates them for attention), so the double-stream blocks, the joint
//    attention and the single-stream blocks need no concat / split copies;
//  * q|k|v (and the single blocks' proj_mlp) are one fused projection; attention reads heads in
//    place and writes straight into the [attn | mlp] operand of proj_out;
//  * all 2*19 + 38 + 1 adaLN modulation linears depend only on temb(t): they are ONE weight matrix
//    [NMOD, D] evaluated for ALL timesteps of the schedule in a single GEMM before the loop
//    (reads 6.5 GB of modulation weights once per image instead of once per step);
//  * bias / GELU / gate*x + residual are GEMM epilogues; LayerNorm+modulate and QK-RMSNorm+RoPE are
//    single-pass row kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "td_kernels.h"
#include "../../include/thinkdiff_hip.h"

namespace {

struct Slot {
  std::string name;
  bf16_t* ptr;
  int64_t count;
  int64_t rows, cols;      // [N, K] of a Linear's weight; [count, 1] of a 1-D parameter
};

// LoRA adapters (td_flux_lora_*; parent context).  An adapter is a set of low-rank pairs, each on one Linear weight slot, kept in the merge kernel's
// operand form (csrc/lora.hip).  Every slot any pair touches holds a BASE COPY of the parameter as it was before the first pair arrived: the
// effective weight in the arena is always recomputed from it, never updated incrementally.
struct LoraPair {
  int slot;
  int rank;
  float scale;             // lora_alpha / rank
  bf16_t* packed;          // At [K, r_pad] | Bp [N, r_pad]
  int64_t bytes;
};
struct LoraAdapter {
  std::string name;
  std::vector<LoraPair> pairs;
  bool active = false;
  float weight = 0.f;
};
struct LoraState {
  std::vector<LoraAdapter> adapters;
  std::unordered_map<int, bf16_t*> base;      // slot -> base copy
};

struct DoubleW {
  bf16_t *qkv_img_w, *qkv_img_b, *qkv_ctx_w, *qkv_ctx_b;
  bf16_t *out_img_w, *out_img_b, *out_ctx_w, *out_ctx_b;
  bf16_t *ff1_img_w, *ff1_img_b, *ff2_img_w, *ff2_img_b;
  bf16_t *ff1_ctx_w, *ff1_ctx_b, *ff2_ctx_w, *ff2_ctx_b;
  bf16_t *norm_q, *norm_k, *norm_added_q, *norm_added_k;
};
struct SingleW {
  bf16_t *w1, *b1;  // [3D + M, D] = to_q | to_k | to_v | proj_mlp
  bf16_t *w2, *b2;  // proj_out [D, D + M]
  bf16_t *norm_q, *norm_k;
};
// fp8 mode (td_flux_set_precision): e4m3 copy of a block weight [rows, K] + one dequantisation scale per output channel
struct Fp8Mat {
  uint8_t* q = nullptr;
  float* s = nullptr;
};
struct DoubleW8 { Fp8Mat qkv_img, qkv_ctx, out_img, out_ctx, ff1_img, ff1_ctx, ff2_img, ff2_ctx; };
// int8 smoothing: the Linears fed by a LayerNorm output (q|k|v, ff.net.0, proj_mlp | q|k|v of the single blocks) may carry up to SM_EXT replicated
// input channels behind their D real ones (one more k-tile); their int8 weights and the quantised LayerNorm rows are allocated for D + SM_EXT
constexpr int SM_EXT = 128;
struct SingleW8 { Fp8Mat w1, w2; };

}  // namespace

struct td_flux {
  TdFluxConfig cfg;
  int D = 0, M = 0, NMOD = 0;
  int max_img = 0, max_txt = 0, max_steps = 0;
  // weights
  bf16_t* arena = nullptr;
  int64_t arena_elems = 0;
  std::vector<Slot> slots;
  std::unordered_map<std::string, int> index;
  bf16_t *x_w, *x_b, *ctx_w, *ctx_b, *t1_w, *t1_b, *t2_w, *t2_b, *g1_w, *g1_b, *g2_w, *g2_b, *p1_w, *p1_b, *p2_w, *p2_b;
  bf16_t *mod_w, *mod_b, *proj_w, *proj_b;
  std::vector<DoubleW> dbl;
  std::vector<SingleW> sgl;
  // Upper bounds of the attention scores of each block (bf16 attention: TdAttnParams::score_bound), from its QK-RMSNorm weights: the norm
  // leaves |q'|, |k| <= sqrt(128) x max|w|, so q'.k <= premul x 128 x max|w_q| x max|w_k|.  Root context; refreshed lazily after weights change.
  std::vector<float> dbl_bound, sgl_bound;
  bool bounds_dirty = true;
  // workspace
  char* ws = nullptr;
  bf16_t *h, *xn, *qkv, *attn, *mlp, *cat, *ctx, *vout;
  bf16_t *tproj, *tmid, *te, *gproj, *gmid, *ge, *pmid, *pe, *temb, *st, *mods;
  float *cosT, *sinT, *ids, *tvals;
  // fp8 mode: quantised block weights, quantised activation rows (xq: LayerNorm output, aq: attention / MLP output)
  int precision = TD_PRECISION_BF16;
  unsigned fp8_mask = TD_FP8_ALL_GEMMS;   // which block Linears run on the fp8 path in fp8 mode (td_flux_set_fp8_gemms)
  char* arena8 = nullptr;
  std::vector<DoubleW8> dbl8;
  std::vector<SingleW8> sgl8;
  uint8_t *xq = nullptr, *aq = nullptr;     // per-context, part of the workspace
  char* attn_ws = nullptr;                  // hand-off workspace of the persistent attention kernel (per context: contexts run concurrently)
  int attn_variant = 0;                     // 0: persistent (stream-K) joint attention; 1: one workgroup per (query tile, head) item
  bool shared_chip = false;                 // several images in flight (td_flux_denoise_multi): kernels of other contexts fill this one's empty rounds
  int attn_mode = 0;                        // parent: TD_ATTENTION_BF16 / TD_ATTENTION_FP8 (td_flux_set_attention)
  char* attn8_ws = nullptr;                 // packed e4m3 q | k | v^T of the 8-bit attention (per context)
  // 8-bit attention, history reference points (TdAttnParams::ref_in / ref_out): per (block, head, token) where the softmax of the NEXT denoise step
  // starts -- two buffers, read / written in turn (a launch reads one and max-accumulates into the other)
  int* href[2] = {nullptr, nullptr};
  int href_cur = 0, href_step = -1, href_T = 0, href_S = 0;      // href[href_cur] holds the references step `href_step` produced for this token layout
  // History (href, hs_*) is the previous step's state OF THE SAME IMAGE UNDER THE SAME NUMERIC CONFIGURATION: set_condition / set_timesteps forget it on
  // their context; every setter that changes weights, precision, Linear classes, scale mode or attention mode bumps the parent's `hist_epoch`, and a
  // context trusts its history only when it was recorded in the current epoch.
  int hist_epoch = 0;                       // parent
  int href_epoch = -1, hs_epoch = -1;       // per context: the epoch href / hs_amax were recorded in
  std::vector<float> tv_host;               // host staging of the schedule scalars (td_flux_set_timesteps)
  float *xs = nullptr, *as_ = nullptr;
  // int8 with history scales (td_flux_set_act_scales): per (block tensor, token) the scale / inverse scale of THIS step, taken from the maxima the
  // previous step accumulated (hs_amax, float bits) -- tensors: MLP input of double block i = [i], [attn | mlp] operand of single block i = [L + i],
  // attention output of double block i = [L + Ls + i]
  int act_scale_mode = 0;                   // parent: 0 = per-token scales measured on the spot (a pass per tensor), 1 = history
  float *hs_scale = nullptr, *hs_inv = nullptr;
  unsigned* hs_amax = nullptr;
  int hs_cap = 0;                           // tokens per tensor in the three arrays
  int hs_step = -1, hs_T = 0, hs_S = 0;     // the step (and token layout) whose maxima hs_amax holds
  // int8 smoothing (td_flux_set_smoothing; parent context).  Per input channel of the Linears that read a LayerNorm output or an MLP intermediate,
  // a power-of-two factor s: the activation channel is divided by s where it is quantised, the weight's input channel multiplied by s before ITS
  // quantisation.  The factors come from ONE calibration forward (the first forward after the mode / the weights / the precision changed, run on the
  // bf16 path with per-channel maxima collected along the way).  Layout of every vector below, in channels: double block i at i (4 D + 2 M):
  // qkv_img[D] qkv_ctx[D] ff1_img[D] ff1_ctx[D] ff2_img[M] ff2_ctx[M]; single block i at L (4 D + 2 M) + i (2 D + M): w1[D] w2[D + M] (the
  // attention half of w2's operand is never smoothed: its maxima stay 0 and its factors 1).
  int smooth_mode = 0;
  bool smooth_ready = false;
  int* sm_ext = nullptr;                            // replicated channels of the LayerNorm-fed Linears: [4 L + Ls tensors][SM_EXT] source channel or -1
  int64_t smooth_n = 0;
  unsigned *sm_ax = nullptr, *sm_aw = nullptr;      // channel maxima of the activations / of the weights' input channels (float bits)
  float *sm_s = nullptr, *sm_inv = nullptr;         // s, 1 / s
  bf16_t* sm_inv16 = nullptr;                       // 1 / s as bf16 (the LayerNorm and GEMM epilogue kernels read it beside their bf16 operands)
  // a forked context (td_flux_fork) shares the parent's weights (bf16 arena, fp8 arena, precision) and owns its
  // workspace, conditioning and schedule: several images in flight on separate streams fill each other's kernel tails
  td_flux* parent = nullptr;
  // LoRA registry (parent only; a fork's copy of the pointer is never used) and the weight epoch: td_flux_lora_set_adapters / delete / clear bump
  // it on the parent, td_flux_set_condition / td_flux_set_timesteps record it on their context (both precompute values from weights), and a
  // forward refuses a context prepared under an older one.
  LoraState* lora = nullptr;
  int weight_epoch = 0;
  int cond_epoch = 0, sched_epoch = 0;
  // state
  int T = 0, S_img = 0, n_steps = 0;
  bool cond_set = false;
  // channel conditioning (FLUX.1 Fill / Canny / Depth): x_embedder reads Cin = Cout + Ccond columns, everything from proj_out on has Cout.
  // xin [max_img, Cin] is the per-context operand of x_embedder: the latents are gathered into its first Cout columns at the head of every
  // forward, td_flux_set_channel_condition writes the rest once per image.  Ccond == 0: no xin, the forward reads the caller's latents.
  int Cin = 0, Cout = 0, Ccond = 0;
  bf16_t* xin = nullptr;
  bool ccond_set = false;
  // reference tokens (FLUX.1 Kontext): S_ref rows that join the image stream behind the S_img latent rows in every forward, constant over the
  // schedule, never stepped or returned.  xref [max_img, Cout] is the per-context operand of x_embedder while S_ref > 0: rows S_img ..
  // S_img + S_ref are written once per image (td_flux_set_reference_tokens), the head rows take the caller's latents by one device-to-device
  // copy per forward.  The blocks then run over T + S_img + S_ref rows; the final norm, proj_out, the velocity and every step kernel keep S_img.
  int S_ref = 0;
  bf16_t* xref = nullptr;
  // optional per-launch HIP-event trace (bench.py roofline leg)
  bool tracing = false;
  std::vector<hipEvent_t> ev_pool;
  struct TraceRec { int cat; double flops; };
  std::vector<TraceRec> trace;
};

namespace {

struct ArenaPlan {
  int64_t off = 0;
  std::vector<std::pair<bf16_t**, int64_t>> fix;  // pointer-to-fill, offset
  void take(bf16_t** p, int64_t n) {
    fix.emplace_back(p, off);
    off += (n + 127) & ~int64_t(127);  // 256-byte aligned tensors
  }
};

void add_slot(td_flux* f, const std::string& name, bf16_t* ptr, int64_t count) {
  f->index[name] = (int)f->slots.size();
  f->slots.push_back({name, ptr, count, count, 1});
}

// registers "<name>.weight" / "<name>.bias" of a Linear living at rows [row0, row0+out) of a fused matrix
void add_linear(td_flux* f, const std::string& name, bf16_t* w, bf16_t* b, int64_t row0, int64_t out, int64_t in) {
  add_slot(f, name + ".weight", w + row0 * in, out * in);
  f->slots.back().rows = out; f->slots.back().cols = in;
  add_slot(f, name + ".bias", b + row0, out);
}

// Brackets one launch with HIP events on ITS stream when tracing is on (categories: TD_TRACE_*).
struct TraceScope {
  td_flux* f; hipStream_t s; bool on;
  TraceScope(td_flux* f_, hipStream_t s_, int cat, double flops) : f(f_), s(s_), on(f_->tracing) {
    if (!on) return;
    const size_t i = f->trace.size();
    if (2 * i + 1 >= f->ev_pool.size()) { on = false; return; }
    f->trace.push_back({cat, flops});
    (void)hipEventRecord(f->ev_pool[2 * i], s);
  }
  ~TraceScope() {
    if (on) (void)hipEventRecord(f->ev_pool[2 * (f->trace.size() - 1) + 1], s);
  }
};

// With several images in flight the partial last round of a GEMM is filled by the other images' kernels, and the tail split's smaller sub-tiles
// only cost (same-box A/B, 2 in flight: bf16 0.580 with the split vs 0.583 without, int8 0.964 vs 0.968): the engine then asks for plain launches.
int gemm_p(td_flux* f, hipStream_t s, const TdGemmParams& p0) {
  TdGemmParams p = p0;
  p.no_tail = f->shared_chip;
  const int cfg = p.cfg >= 0 ? p.cfg : td_gemm_config_id(p.M + p.g_M, p.N, p.K);
  TraceScope ts(f, s, cfg == 0 ? TD_TRACE_GEMM_MAIN : cfg == 3 ? TD_TRACE_GEMM_288 : TD_TRACE_GEMM_OTHER, 2.0 * (p.M + p.g_M) * p.N * p.K);
  return td_gemm_launch(p, s);
}

int gemm(td_flux* f, hipStream_t s, const bf16_t* A, int lda, const bf16_t* W, const bf16_t* b, bf16_t* C, int ldc,
         int M, int N, int K, int act = TD_ACT_NONE, const bf16_t* gate = nullptr, const bf16_t* res = nullptr, int ldr = 0) {
  TdGemmParams p;
  p.A = A; p.lda = lda; p.W = W; p.bias = b; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  p.act = act; p.gate = gate; p.res = res; p.ldr = ldr;
  return gemm_p(f, s, p);
}

// image-stream + text-stream Linear of a double block in one launch (problem 0 = image rows)
int gemm2(td_flux* f, hipStream_t s, const bf16_t* A0, const bf16_t* W0, const bf16_t* b0, bf16_t* C0, int M0,
          const bf16_t* A1, const bf16_t* W1, const bf16_t* b1, bf16_t* C1, int M1, int ld_a, int ld_c, int N, int K,
          int act = TD_ACT_NONE, const bf16_t* gate0 = nullptr, const bf16_t* gate1 = nullptr, bool residual = false) {
  TdGemmParams p;
  p.A = A0; p.W = W0; p.bias = b0; p.C = C0; p.M = M0; p.gate = gate0; p.res = residual ? C0 : nullptr;
  p.g_A = A1; p.g_W = W1; p.g_bias = b1; p.g_C = C1; p.g_M = M1; p.g_gate = gate1; p.g_res = residual ? C1 : nullptr;
  p.lda = ld_a; p.ldc = ld_c; p.ldr = ld_c; p.N = N; p.K = K; p.act = act;
  return gemm_p(f, s, p);
}

// fp8 forms of gemm / gemm2: A is e4m3 rows + per-row scales, W an Fp8Mat
// int8 output of the activated result under scales fixed in advance (TdGemmParams::q8)
struct Q8Out { uint8_t* q = nullptr; int ld = 0; const float* inv = nullptr; unsigned* amax = nullptr; const bf16_t* smooth = nullptr; };

int gemm8(td_flux* f, hipStream_t s, const uint8_t* A, int lda, const float* a_scale, const Fp8Mat& W, const bf16_t* b, bf16_t* C, int ldc,
          int M, int N, int K, int act = TD_ACT_NONE, const bf16_t* gate = nullptr, const bf16_t* res = nullptr, int ldr = 0,
          bf16_t* C2 = nullptr, int ldc2 = 0, int act2 = TD_ACT_NONE, int n_split = 0, const Q8Out* q8 = nullptr) {
  TdGemmParams p;
  const td_flux* root8 = f->parent ? f->parent : f;
  p.fp8 = root8->precision == TD_PRECISION_FP8_E4M3; p.i8 = root8->precision == TD_PRECISION_INT8;
  p.A = (const bf16_t*)A; p.lda = lda; p.a_scale = a_scale; p.W = (const bf16_t*)W.q; p.w_scale = W.s;
  p.bias = b; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.act = act; p.gate = gate; p.res = res; p.ldr = ldr;
  p.C2 = C2; p.ldc2 = ldc2; p.act2 = act2; p.n_split = n_split;
  if (q8) { p.q8 = q8->q; p.ldq8 = q8->ld; p.q8_inv = q8->inv; p.q8_amax = q8->amax; p.q8_smooth = q8->smooth; }
  p.no_tail = f->shared_chip;
  const int cfg = td_gemm_config_id(M, N, K / 2);
  TraceScope ts(f, s, cfg == 0 ? TD_TRACE_GEMM_MAIN : cfg == 3 ? TD_TRACE_GEMM_288 : TD_TRACE_GEMM_OTHER, 2.0 * M * N * K);
  return td_gemm_launch(p, s);
}
int gemm2_8(td_flux* f, hipStream_t s, const uint8_t* A0, const float* as0, const Fp8Mat& W0, const bf16_t* b0, bf16_t* C0, int M0,
            const uint8_t* A1, const float* as1, const Fp8Mat& W1, const bf16_t* b1, bf16_t* C1, int M1, int ld_a, int ld_c, int N, int K,
            int act = TD_ACT_NONE, const bf16_t* gate0 = nullptr, const bf16_t* gate1 = nullptr, bool residual = false,
            const Q8Out* q8_0 = nullptr, const Q8Out* q8_1 = nullptr) {
  TdGemmParams p;
  if (q8_0 && q8_1) {
    p.q8 = q8_0->q; p.ldq8 = q8_0->ld; p.q8_inv = q8_0->inv; p.q8_amax = q8_0->amax; p.q8_smooth = q8_0->smooth;
    p.g_q8 = q8_1->q; p.g_q8_inv = q8_1->inv; p.g_q8_amax = q8_1->amax; p.g_q8_smooth = q8_1->smooth;
  }
  const td_flux* root8 = f->parent ? f->parent : f;
  p.fp8 = root8->precision == TD_PRECISION_FP8_E4M3; p.i8 = root8->precision == TD_PRECISION_INT8;
  p.A = (const bf16_t*)A0; p.a_scale = as0; p.W = (const bf16_t*)W0.q; p.w_scale = W0.s; p.bias = b0; p.C = C0; p.M = M0;
  p.gate = gate0; p.res = residual ? C0 : nullptr;
  p.g_A = (const bf16_t*)A1; p.g_a_scale = as1; p.g_W = (const bf16_t*)W1.q; p.g_w_scale = W1.s; p.g_bias = b1; p.g_C = C1; p.g_M = M1;
  p.g_gate = gate1; p.g_res = residual ? C1 : nullptr;
  p.lda = ld_a; p.ldc = ld_c; p.ldr = ld_c; p.N = N; p.K = K; p.act = act;
  p.no_tail = f->shared_chip;
  const int cfg = td_gemm_config_id(M0 + M1, N, K / 2);
  TraceScope ts(f, s, cfg == 0 ? TD_TRACE_GEMM_MAIN : cfg == 3 ? TD_TRACE_GEMM_288 : TD_TRACE_GEMM_OTHER, 2.0 * (M0 + M1) * N * K);
  return td_gemm_launch(p, s);
}
// per-token quantisation of a bf16 activation matrix into f->aq / f->as_ (rows row0 .. row0 + rows - 1 of both); col_mul: int8 smoothing factors (1 / s)
int quant_act(td_flux* f, hipStream_t s, const bf16_t* x, int ldx, int rows, int K, unsigned* amax_out = nullptr, const float* col_mul = nullptr, int row0 = 0) {
  TraceScope ts(f, s, TD_TRACE_NORM, 0.0);
  return td_quant_rows_fp8_launch(x + (size_t)row0 * ldx, ldx, f->aq + (size_t)row0 * K, K, f->as_ + row0, rows, K, s,
                                  (f->parent ? f->parent : f)->precision == TD_PRECISION_INT8, amax_out ? amax_out + row0 : nullptr, col_mul);
}

int norm_rows(td_flux* f, hipStream_t s, const TdNormParams& p) {
  TraceScope ts(f, s, TD_TRACE_NORM, 0.0);
  return td_norm_rows_launch(p, s);
}
int qk_rope(td_flux* f, hipStream_t s, const TdQkRopeParams& p) {
  TraceScope ts(f, s, TD_TRACE_QKROPE, 0.0);
  return td_qk_norm_rope_launch(p, s);
}
// rope != null: the 8-bit attention's pack pass applies QK-RMSNorm + RoPE itself (the block loop skipped td_qk_norm_rope)
int attn(td_flux* f, hipStream_t s, const TdAttnParams& p, const TdQkRopeParams* rope = nullptr, const int* ref_in = nullptr, int* ref_out = nullptr) {
  TraceScope ts(f, s, TD_TRACE_ATTN, 4.0 * p.Sq * (double)p.Skv * p.Hq * 128.0);
  const td_flux* root = f->parent ? f->parent : f;
  if (root->attn_mode == TD_ATTENTION_FP8) {      // both products on the e4m3 MFMA: pack pass + persistent kernel (csrc/attention_fp8.hip)
    TdAttnParams q = p;
    q.f8_ws = f->attn8_ws;
    q.variant = p.variant & 0x1000;
    q.ref_in = ref_in; q.ref_out = ref_out;
    if (rope) {
      const TdQkRopeParams& r = *rope;
      q.rope_cos = r.cos; q.rope_sin = r.sin; q.rope_split = r.split; q.rope_eps = r.eps; q.rope_q_premul = r.q_premul;
      q.rope_wqA = r.wqA; q.rope_wkA = r.wkA; q.rope_wqB = r.wqB; q.rope_wkB = r.wkB;
    }
    return td_attn_fp8_launch(q, s);
  }
  return td_attn_launch(p, s);
}

// N may exceed the 4 GiB buffer-descriptor range of W (the fused modulation matrix is 6.5 GB):
// walk it in column chunks.
int gemm_big_n(td_flux* f, hipStream_t s, const bf16_t* A, int lda, const bf16_t* W, const bf16_t* b, bf16_t* C, int ldc,
               int M, int64_t N, int K) {
  const int64_t chunk = 131072;
  for (int64_t n0 = 0; n0 < N; n0 += chunk) {
    const int nn = (int)(N - n0 < chunk ? N - n0 : chunk);
    int rc = gemm(f, s, A, lda, W + n0 * K, b + n0, C + n0, ldc, M, nn, K);
    if (rc != 0) return rc;
  }
  return 0;
}

#define TD_TRY(expr)          \
  do {                        \
    int _rc = (expr);         \
    if (_rc != 0) return _rc; \
  } while (0)

// per-context activation workspace (one allocation)
int alloc_workspace(td_flux* f) {
  // ---- activation workspace -----------------------------------------------------------------------
  const TdFluxConfig* cfg = &f->cfg;
  const int64_t D = f->D, M = f->M;
  const int max_img_tokens = f->max_img, max_txt_tokens = f->max_txt;
  const int64_t S = (int64_t)max_img_tokens + max_txt_tokens;
  const int64_t n = f->max_steps;
  struct Req { void** p; int64_t bytes; };
  std::vector<Req> reqs = {
      {(void**)&f->h, S * D * 2}, {(void**)&f->xn, S * D * 2}, {(void**)&f->qkv, S * 3 * D * 2},
      {(void**)&f->attn, S * D * 2}, {(void**)&f->mlp, S * M * 2}, {(void**)&f->cat, S * (D + M) * 2},
      {(void**)&f->ctx, (int64_t)max_txt_tokens * D * 2}, {(void**)&f->vout, (int64_t)max_img_tokens * f->Cout * 2},
      {(void**)&f->xin, f->Ccond > 0 ? (int64_t)max_img_tokens * f->Cin * 2 : 0},
      {(void**)&f->xref, f->Ccond == 0 ? (int64_t)max_img_tokens * f->Cout * 2 : 0},
      {(void**)&f->tproj, n * 256 * 2}, {(void**)&f->tmid, n * D * 2}, {(void**)&f->te, n * D * 2},
      {(void**)&f->gproj, 256 * 2}, {(void**)&f->gmid, (int64_t)D * 2}, {(void**)&f->ge, (int64_t)D * 2},
      {(void**)&f->pmid, (int64_t)D * 2}, {(void**)&f->pe, (int64_t)D * 2},
      {(void**)&f->temb, n * D * 2}, {(void**)&f->st, n * D * 2}, {(void**)&f->mods, n * (int64_t)f->NMOD * 2},
      {(void**)&f->cosT, S * 128 * 4}, {(void**)&f->sinT, S * 128 * 4}, {(void**)&f->ids, S * 3 * 4},
      {(void**)&f->tvals, (n + 1) * 4},
      {(void**)&f->xq, S * (D + SM_EXT)}, {(void**)&f->aq, S * (D + M)}, {(void**)&f->xs, S * 4}, {(void**)&f->as_, S * 4},   // fp8 mode activations
      {(void**)&f->attn_ws, (int64_t)td_attn_streamk_ws_bytes()},
      {(void**)&f->attn8_ws, (int64_t)td_attn_fp8_ws_bytes((int)S, (int)S, cfg->num_heads)},
      {(void**)&f->href[0], (int64_t)(cfg->num_layers + cfg->num_single_layers) * cfg->num_heads * S * 4},
      {(void**)&f->href[1], (int64_t)(cfg->num_layers + cfg->num_single_layers) * cfg->num_heads * S * 4},
      {(void**)&f->hs_scale, (int64_t)(2 * cfg->num_layers + cfg->num_single_layers) * S * 4}, {(void**)&f->hs_inv, (int64_t)(2 * cfg->num_layers + cfg->num_single_layers) * S * 4},
      {(void**)&f->hs_amax, (int64_t)(2 * cfg->num_layers + cfg->num_single_layers) * S * 4},
  };
  f->hs_cap = (int)S;
  f->hs_step = -1;
  f->href_step = -1;
  int64_t total = 0;
  for (auto& r : reqs) total += (r.bytes + 255) & ~int64_t(255);
  hipError_t e = hipMalloc((void**)&f->ws, (size_t)total);
  if (e != hipSuccess) {
    td_set_error("td_flux: hipMalloc of %.2f GiB workspace failed: %s", total / double(1 << 30), hipGetErrorString(e));
    return TD_ERR_HIP;
  }
  (void)hipMemset(f->ws, 0, (size_t)total);
  (void)hipDeviceSynchronize();   // the handle may be used from any stream next; a null-stream memset is not ordered with non-blocking streams
  int64_t o = 0;
  for (auto& r : reqs) {
    *r.p = r.bytes ? f->ws + o : nullptr;
    o += (r.bytes + 255) & ~int64_t(255);
  }
  return TD_OK;
}

}  // namespace

extern "C" {

int td_flux_create(const TdFluxConfig* cfg, int max_img_tokens, int max_txt_tokens, int max_steps, td_flux** out) {
  TD_CHECK_ARG(cfg && out, "td_flux_create: null argument");
  TD_CHECK_ARG(cfg->head_dim == 128, "td_flux_create: head_dim must be 128");
  TD_CHECK_ARG(cfg->axes_dims[0] + cfg->axes_dims[1] + cfg->axes_dims[2] == 128, "td_flux_create: rope axes must sum to 128");
  TD_CHECK_ARG(cfg->in_channels % 64 == 0 && cfg->joint_dim % 64 == 0 && cfg->pooled_dim % 64 == 0, "td_flux_create: input widths must be multiples of 64");
  TD_CHECK_ARG((cfg->num_heads * 128) % 512 == 0, "td_flux_create: inner dim must be a multiple of 512");
  TD_CHECK_ARG(max_img_tokens > 0 && max_txt_tokens > 0 && max_steps > 0, "td_flux_create: capacities must be positive");
  const int c_out = cfg->out_channels ? cfg->out_channels : cfg->in_channels;
  TD_CHECK_ARG(cfg->in_channels > 0 && c_out > 0 && c_out % 64 == 0, "td_flux_create: in_channels=%d, out_channels=%d must be positive multiples of 64",
               cfg->in_channels, c_out);
  TD_CHECK_ARG(c_out <= cfg->in_channels, "td_flux_create: out_channels=%d exceeds in_channels=%d (in_channels = out_channels + the channel condition's width)",
               c_out, cfg->in_channels);
  td_flux* f = new td_flux();
  f->cfg = *cfg;
  f->cfg.out_channels = c_out;
  f->Cin = cfg->in_channels; f->Cout = c_out; f->Ccond = cfg->in_channels - c_out;
  const int D = f->D = cfg->num_heads * cfg->head_dim;
  const int M = f->M = cfg->mlp_ratio * D;
  const int L = cfg->num_layers, Ls = cfg->num_single_layers;
  f->NMOD = L * 12 * D + Ls * 3 * D + 2 * D;
  f->max_img = max_img_tokens; f->max_txt = max_txt_tokens; f->max_steps = max_steps;
  f->dbl.resize(L);
  f->sgl.resize(Ls);

  // ---- weight arena ---------------------------------------------------------------------------
  ArenaPlan ap;
  ap.take(&f->x_w, (int64_t)D * cfg->in_channels); ap.take(&f->x_b, D);
  ap.take(&f->ctx_w, (int64_t)D * cfg->joint_dim); ap.take(&f->ctx_b, D);
  ap.take(&f->t1_w, (int64_t)D * 256); ap.take(&f->t1_b, D);
  ap.take(&f->t2_w, (int64_t)D * D); ap.take(&f->t2_b, D);
  ap.take(&f->g1_w, (int64_t)D * 256); ap.take(&f->g1_b, D);
  ap.take(&f->g2_w, (int64_t)D * D); ap.take(&f->g2_b, D);
  ap.take(&f->p1_w, (int64_t)D * cfg->pooled_dim); ap.take(&f->p1_b, D);
  ap.take(&f->p2_w, (int64_t)D * D); ap.take(&f->p2_b, D);
  ap.take(&f->mod_w, (int64_t)f->NMOD * D); ap.take(&f->mod_b, f->NMOD);
  ap.take(&f->proj_w, (int64_t)f->Cout * D); ap.take(&f->proj_b, f->Cout);
  for (auto& w : f->dbl) {
    ap.take(&w.qkv_img_w, (int64_t)3 * D * D); ap.take(&w.qkv_img_b, 3 * D);
    ap.take(&w.qkv_ctx_w, (int64_t)3 * D * D); ap.take(&w.qkv_ctx_b, 3 * D);
    ap.take(&w.out_img_w, (int64_t)D * D); ap.take(&w.out_img_b, D);
    ap.take(&w.out_ctx_w, (int64_t)D * D); ap.take(&w.out_ctx_b, D);
    ap.take(&w.ff1_img_w, (int64_t)M * D); ap.take(&w.ff1_img_b, M);
    ap.take(&w.ff2_img_w, (int64_t)D * M); ap.take(&w.ff2_img_b, D);
    ap.take(&w.ff1_ctx_w, (int64_t)M * D); ap.take(&w.ff1_ctx_b, M);
    ap.take(&w.ff2_ctx_w, (int64_t)D * M); ap.take(&w.ff2_ctx_b, D);
    ap.take(&w.norm_q, 128); ap.take(&w.norm_k, 128); ap.take(&w.norm_added_q, 128); ap.take(&w.norm_added_k, 128);
  }
  for (auto& w : f->sgl) {
    ap.take(&w.w1, (int64_t)(3 * D + M) * D); ap.take(&w.b1, 3 * D + M);
    ap.take(&w.w2, (int64_t)D * (D + M)); ap.take(&w.b2, D);
    ap.take(&w.norm_q, 128); ap.take(&w.norm_k, 128);
  }
  f->arena_elems = ap.off;
  hipError_t e = hipMalloc((void**)&f->arena, (size_t)ap.off * sizeof(bf16_t));
  if (e != hipSuccess) {
    td_set_error("td_flux_create: hipMalloc of %.2f GiB weight arena failed: %s", ap.off * 2.0 / (1 << 30), hipGetErrorString(e));
    delete f;
    return TD_ERR_HIP;
  }
  for (auto& fx : ap.fix) *fx.first = f->arena + fx.second;

  // ---- parameter table under the diffusers state-dict names ----------------------------------------
  add_linear(f, "x_embedder", f->x_w, f->x_b, 0, D, cfg->in_channels);
  add_linear(f, "context_embedder", f->ctx_w, f->ctx_b, 0, D, cfg->joint_dim);
  add_linear(f, "time_text_embed.timestep_embedder.linear_1", f->t1_w, f->t1_b, 0, D, 256);
  add_linear(f, "time_text_embed.timestep_embedder.linear_2", f->t2_w, f->t2_b, 0, D, D);
  if (cfg->guidance_embeds) {
    add_linear(f, "time_text_embed.guidance_embedder.linear_1", f->g1_w, f->g1_b, 0, D, 256);
    add_linear(f, "time_text_embed.guidance_embedder.linear_2", f->g2_w, f->g2_b, 0, D, D);
  }
  add_linear(f, "time_text_embed.text_embedder.linear_1", f->p1_w, f->p1_b, 0, D, cfg->pooled_dim);
  add_linear(f, "time_text_embed.text_embedder.linear_2", f->p2_w, f->p2_b, 0, D, D);
  for (int i = 0; i < L; ++i) {
    const std::string p = "transformer_blocks." + std::to_string(i) + ".";
    DoubleW& w = f->dbl[i];
    add_linear(f, p + "norm1.linear", f->mod_w, f->mod_b, (int64_t)i * 12 * D, 6 * D, D);
    add_linear(f, p + "norm1_context.linear", f->mod_w, f->mod_b, (int64_t)i * 12 * D + 6 * D, 6 * D, D);
    add_linear(f, p + "attn.to_q", w.qkv_img_w, w.qkv_img_b, 0, D, D);
    add_linear(f, p + "attn.to_k", w.qkv_img_w, w.qkv_img_b, D, D, D);
    add_linear(f, p + "attn.to_v", w.qkv_img_w, w.qkv_img_b, 2 * D, D, D);
    add_linear(f, p + "attn.add_q_proj", w.qkv_ctx_w, w.qkv_ctx_b, 0, D, D);
    add_linear(f, p + "attn.add_k_proj", w.qkv_ctx_w, w.qkv_ctx_b, D, D, D);
    add_linear(f, p + "attn.add_v_proj", w.qkv_ctx_w, w.qkv_ctx_b, 2 * D, D, D);
    add_linear(f, p + "attn.to_out.0", w.out_img_w, w.out_img_b, 0, D, D);
    add_linear(f, p + "attn.to_add_out", w.out_ctx_w, w.out_ctx_b, 0, D, D);
    add_slot(f, p + "attn.norm_q.weight", w.norm_q, 128);
    add_slot(f, p + "attn.norm_k.weight", w.norm_k, 128);
    add_slot(f, p + "attn.norm_added_q.weight", w.norm_added_q, 128);
    add_slot(f, p + "attn.norm_added_k.weight", w.norm_added_k, 128);
    add_linear(f, p + "ff.net.0.proj", w.ff1_img_w, w.ff1_img_b, 0, M, D);
    add_linear(f, p + "ff.net.2", w.ff2_img_w, w.ff2_img_b, 0, D, M);
    add_linear(f, p + "ff_context.net.0.proj", w.ff1_ctx_w, w.ff1_ctx_b, 0, M, D);
    add_linear(f, p + "ff_context.net.2", w.ff2_ctx_w, w.ff2_ctx_b, 0, D, M);
  }
  for (int i = 0; i < Ls; ++i) {
    const std::string p = "single_transformer_blocks." + std::to_string(i) + ".";
    SingleW& w = f->sgl[i];
    add_linear(f, p + "norm.linear", f->mod_w, f->mod_b, (int64_t)L * 12 * D + (int64_t)i * 3 * D, 3 * D, D);
    add_linear(f, p + "attn.to_q", w.w1, w.b1, 0, D, D);
    add_linear(f, p + "attn.to_k", w.w1, w.b1, D, D, D);
    add_linear(f, p + "attn.to_v", w.w1, w.b1, 2 * D, D, D);
    add_linear(f, p + "proj_mlp", w.w1, w.b1, 3 * D, M, D);
    add_linear(f, p + "proj_out", w.w2, w.b2, 0, D, D + M);
    add_slot(f, p + "attn.norm_q.weight", w.norm_q, 128);
    add_slot(f, p + "attn.norm_k.weight", w.norm_k, 128);
  }
  add_linear(f, "norm_out.linear", f->mod_w, f->mod_b, (int64_t)L * 12 * D + (int64_t)Ls * 3 * D, 2 * D, D);
  add_linear(f, "proj_out", f->proj_w, f->proj_b, 0, f->Cout, D);

  if (int rc = alloc_workspace(f)) {
    (void)hipFree(f->arena);
    delete f;
    return rc;
  }
  *out = f;
  return TD_OK;
}

void td_flux_destroy(td_flux* f) {
  if (!f) return;
  for (hipEvent_t ev : f->ev_pool) (void)hipEventDestroy(ev);
  if (!f->parent) {
    if (f->lora) {
      for (auto& a : f->lora->adapters) for (auto& p : a.pairs) (void)hipFree(p.packed);
      for (auto& b : f->lora->base) (void)hipFree(b.second);
      delete f->lora;
    }
    (void)hipFree(f->arena);
    if (f->arena8) (void)hipFree(f->arena8);
    if (f->sm_ax) (void)hipFree(f->sm_ax);      // one allocation: ax | aw | s | inv | inv16
    if (f->sm_ext) (void)hipFree(f->sm_ext);
  }
  (void)hipFree(f->ws);
  delete f;
}

// A second context over the same weights: own workspace / conditioning / timestep schedule, so that independent images
// can be in flight on separate streams.  The parent must outlive its forks; precision and parameters are the parent's.
int td_flux_fork(td_flux* src, td_flux** out) {
  TD_CHECK_ARG(src && out, "td_flux_fork: null argument");
  td_flux* root = src->parent ? src->parent : src;
  td_flux* f = new td_flux(*root);
  f->parent = root;
  f->ws = nullptr;
  f->ev_pool.clear(); f->trace.clear(); f->tracing = false;
  f->T = f->S_img = f->n_steps = 0; f->cond_set = false; f->ccond_set = false; f->S_ref = 0;
  if (int rc = alloc_workspace(f)) { delete f; return rc; }
  *out = f;
  return TD_OK;
}

int64_t td_flux_param_elems(const td_flux* f) { return f ? f->arena_elems : 0; }
int td_flux_num_params(const td_flux* f) { return f ? (int)f->slots.size() : 0; }

int td_flux_param_info(const td_flux* f, int idx, char* name_buf, int buf_len, int64_t* count) {
  TD_CHECK_ARG(f && idx >= 0 && idx < (int)f->slots.size(), "td_flux_param_info: index %d out of range", idx);
  const Slot& s = f->slots[idx];
  if (name_buf && buf_len > 0) {
    strncpy(name_buf, s.name.c_str(), buf_len - 1);
    name_buf[buf_len - 1] = 0;
  }
  if (count) *count = s.count;
  return TD_OK;
}

// Host copy of a 128-element norm weight -> max |w| (synchronous: called once per weight change, behind a device synchronise)
static int norm_weight_max(const bf16_t* w, float* out) {
  uint16_t h[128];
  TD_CHECK_HIP(hipMemcpy(h, w, sizeof(h), hipMemcpyDeviceToHost));
  float m = 0.f;
  for (int i = 0; i < 128; ++i) {
    const uint32_t u = (uint32_t)h[i] << 16;
    float v;
    memcpy(&v, &u, 4);
    v = fabsf(v);
    if (!(v <= 3.0e38f)) v = 3.0e38f;      // NaN / inf weights: no bound
    m = fmaxf(m, v);
  }
  *out = m;
  return TD_OK;
}
// A bound is used only up to 48 octaves: the attention then exponentiates the scores as they are (|s| <= bound: exp2(s) and its sums stay far inside fp32).
static int refresh_score_bounds(td_flux* root) {
  TD_CHECK_HIP(hipDeviceSynchronize());      // weight loads ran on the callers' streams
  const float c = 0.08838834764831845f * 1.4426950408889634f * 128.0f * 1.02f;      // premul x head_dim, 2 % for the bf16 roundings of q' and k
  constexpr float LIMIT = 48.0f;
  root->dbl_bound.assign(root->dbl.size(), 0.f);
  root->sgl_bound.assign(root->sgl.size(), 0.f);
  for (size_t i = 0; i < root->dbl.size(); ++i) {
    float a, b, cq, ck;
    TD_TRY(norm_weight_max(root->dbl[i].norm_q, &a)); TD_TRY(norm_weight_max(root->dbl[i].norm_added_q, &cq));
    TD_TRY(norm_weight_max(root->dbl[i].norm_k, &b)); TD_TRY(norm_weight_max(root->dbl[i].norm_added_k, &ck));
    const float bound = c * fmaxf(a, cq) * fmaxf(b, ck);
    root->dbl_bound[i] = bound > 0.f && bound <= LIMIT ? bound : 0.f;
  }
  for (size_t i = 0; i < root->sgl.size(); ++i) {
    float a, b;
    TD_TRY(norm_weight_max(root->sgl[i].norm_q, &a)); TD_TRY(norm_weight_max(root->sgl[i].norm_k, &b));
    const float bound = c * a * b;
    root->sgl_bound[i] = bound > 0.f && bound <= LIMIT ? bound : 0.f;
  }
  root->bounds_dirty = false;
  return TD_OK;
}

int td_flux_load_param(td_flux* f, const char* name, const void* src, int64_t count, void* stream) {
  TD_CHECK_ARG(f && name && src, "td_flux_load_param: null argument");
  (f->parent ? f->parent : f)->bounds_dirty = true;
  ++(f->parent ? f->parent : f)->hist_epoch;
  (f->parent ? f->parent : f)->smooth_ready = false;
  auto it = f->index.find(name);
  TD_CHECK_ARG(it != f->index.end(), "td_flux_load_param: unknown parameter '%s'", name);
  const Slot& s = f->slots[it->second];
  TD_CHECK_ARG(s.count == count, "td_flux_load_param: '%s' expects %lld elements, got %lld", name, (long long)s.count, (long long)count);
  {
    const LoraState* ls = (f->parent ? f->parent : f)->lora;
    TD_CHECK_ARG(!ls || !ls->base.count(it->second), "td_flux_load_param: '%s' carries LoRA adapters (its base copy would go stale): clear the adapters first "
                 "(td_flux_lora_clear)", name);
  }
  TD_CHECK_HIP(hipMemcpyAsync(s.ptr, src, (size_t)count * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

// fp8 mode: quantise every block Linear (per output channel, OCP e4m3) from the bf16 arena as it stands NOW -- call
// after the checkpoint is loaded, and again after reloading parameters.  Embedders, modulation and the final
// projection stay bf16 (< 0.1 % of the FLOPs; the modulation GEMM runs once per image).
int td_flux_set_fp8_gemms(td_flux* f, unsigned mask) {
  TD_CHECK_ARG(f && !f->parent, "td_flux_set_fp8_gemms: set it on the parent context (forks follow it)");
  TD_CHECK_ARG((mask & ~(unsigned)TD_FP8_ALL_GEMMS) == 0, "td_flux_set_fp8_gemms: unknown bits in mask 0x%x", mask);
  f->fp8_mask = mask;
  ++f->hist_epoch;
  return TD_OK;
}

// TD_PRECISION_INT8 only: where the per-token activation scales of the attention-output / MLP operands come from.  0 (default): measured
// on the spot -- one quantisation pass per tensor.  1: from the maxima the PREVIOUS denoise step accumulated for the same tensor and
// token, times 1.25 (values beyond that clip at +-127): the MLP intermediate then leaves the producing GEMM epilogue as int8 and the
// passes over it disappear; the first step of an image, and any step that does not follow its predecessor, runs the mode-0 path.
int td_flux_set_act_scales(td_flux* f, int mode) {
  TD_CHECK_ARG(f && !f->parent && (mode == 0 || mode == 1), "td_flux_set_act_scales: parent context, mode 0 or 1");
  f->act_scale_mode = mode;
  ++f->hist_epoch;
  return TD_OK;
}

// TD_PRECISION_INT8 only: per-channel smoothing of the activations that carry outlier channels (SmoothQuant's balance, alpha = 1/2, factors rounded
// to powers of two).  Per-token symmetric int8 gives every channel of a row the step max|row| / 127: a trained DiT's few residual-stream /
// MLP channels that run tens of times above the rest then leave the rest 2-3 bits.  With mode 1 the FIRST int8 forward after the mode, the
// precision or a parameter changed runs on the bf16 path and records, per input channel of the Linears fed by a LayerNorm output (q|k|v, ff.net.0,
// proj_mlp) or by an MLP intermediate (ff.net.2, proj_out's MLP half), the largest activation; s = 2^rint(log2 sqrt(max|x_c| / max|W[:, c]|)) then
// divides that activation channel (inside the LayerNorm kernel, the producing GEMM's int8 epilogue or the quantisation pass) and multiplies the
// weight's input channel before the weight is quantised again.  Powers of two: x / s and W s are exact, the product is the unsmoothed one, only
// the quantisation steps move.  0 (default) = off.  Parent context.
int td_flux_set_smoothing(td_flux* f, int mode) {
  TD_CHECK_ARG(f && !f->parent && (mode == 0 || mode == 1), "td_flux_set_smoothing: parent context, mode 0 or 1");
  if (mode == 1 && !f->sm_ax) {
    const int64_t D = f->D, M = f->M;
    const int64_t n = (int64_t)f->cfg.num_layers * (4 * D + 2 * M) + (int64_t)f->cfg.num_single_layers * (2 * D + M);
    char* base = nullptr;
    TD_CHECK_HIP(hipMalloc((void**)&base, (size_t)n * (4 + 4 + 4 + 4 + 2)));
    f->smooth_n = n;
    f->sm_ax = (unsigned*)base; f->sm_aw = f->sm_ax + n; f->sm_s = (float*)(f->sm_aw + n); f->sm_inv = f->sm_s + n; f->sm_inv16 = (bf16_t*)(f->sm_inv + n);
    TD_CHECK_HIP(hipMalloc((void**)&f->sm_ext, (size_t)(4 * f->cfg.num_layers + f->cfg.num_single_layers) * SM_EXT * sizeof(int)));
  }
  if (mode != f->smooth_mode) {
    ++f->hist_epoch;
    f->smooth_ready = false;
    // leaving the mode: the int8 weights must lose their column factors -- quantise them again from the bf16 arena
    if (mode == 0 && f->smooth_mode == 1 && f->precision == TD_PRECISION_INT8 && f->arena8) { f->smooth_mode = 0; return td_flux_set_precision(f, TD_PRECISION_INT8, nullptr); }
  }
  f->smooth_mode = mode;
  return TD_OK;
}

}  // extern "C"

namespace {
inline int64_t sm_dbl(const td_flux* r, int i) { return (int64_t)i * (4 * (int64_t)r->D + 2 * (int64_t)r->M); }
inline int64_t sm_sgl(const td_flux* r, int i) { return (int64_t)r->cfg.num_layers * (4 * (int64_t)r->D + 2 * (int64_t)r->M) + (int64_t)i * (2 * (int64_t)r->D + r->M); }

// Factors of one Linear's input channels from the maxima the calibration forward saw (ax) and the weight's column maxima (aw), on the host.
// A channel is an outlier when its maximum is more than 4 x the median channel's; it is brought down to ~2 x the median by a power of two t:
//   * as far as the weight's own column is SMALLER than the median column (a trained MLP pairs an outlier intermediate channel with small
//     weights), multiplicatively: activation / m, weight column x m -- free, the column only returns to normal size;
//   * what is left, r = t / m, by REPLICATION where the operand has room for it (ext != null: the LayerNorm-fed Linears, SM_EXT spare channels
//     per tensor, largest outliers first): activation / r, present r times, weight column untouched -- the contraction sums r x (x / r) w;
//   * the rest (no room, or an MLP-fed Linear whose weight column is not small) by SmoothQuant's even split: activation / sqrt, weight x sqrt.
// Every other channel keeps factor 1: on a checkpoint without outlier channels the smoothed form IS the plain one.
void smooth_plan(const float* ax, const float* aw, int K, float* s_w, float* inv_a, int* ext) {
  std::vector<float> v;
  for (int c = 0; c < K; ++c) if (ax[c] > 0.f) v.push_back(ax[c]);
  for (int c = 0; c < K; ++c) { s_w[c] = 1.f; inv_a[c] = 1.f; }
  if (ext) for (int e = 0; e < SM_EXT; ++e) ext[e] = -1;
  if (v.size() < 16) return;
  std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
  const float med = v[v.size() / 2];
  std::vector<float> wv;
  for (int c = 0; c < K; ++c) if (aw[c] > 0.f) wv.push_back(aw[c]);
  float wmed = 0.f;
  if (!wv.empty()) { std::nth_element(wv.begin(), wv.begin() + wv.size() / 2, wv.end()); wmed = wv[wv.size() / 2]; }
  auto pow2floor = [](float x) { return x >= 1.f ? std::exp2(std::floor(std::log2(x))) : 1.f; };
  struct Out { int c; float t, m, r; };
  std::vector<Out> outs;
  for (int c = 0; c < K; ++c) {
    if (!(ax[c] > 4.f * med)) continue;
    const float t = std::min(pow2floor(ax[c] / (2.f * med)), 256.f);
    const float m = (aw[c] > 0.f && wmed > 0.f) ? std::min(t, pow2floor(wmed / aw[c])) : 1.f;
    outs.push_back({c, t, m, t / m});
  }
  std::sort(outs.begin(), outs.end(), [](const Out& a, const Out& b) { return a.r > b.r; });
  int room = ext ? SM_EXT : 0, e = 0;
  for (Out& o : outs) {
    float r = o.r;
    while (r > 1.f && (int)r - 1 > room) r *= 0.5f;      // as many copies as still fit
    const float rest = o.r / r;                            // what replication could not take: split evenly (power of two nearest the square root)
    const float half = rest > 1.f ? std::exp2(std::rint(0.5f * std::log2(rest))) : 1.f;
    for (int k = 0; k < (int)r - 1; ++k) ext[e++] = o.c;
    room -= (int)r - 1;
    s_w[o.c] = o.m * half;
    inv_a[o.c] = 1.f / (o.m * r * half);
  }
}

// End of the calibration forward (stream s): the weights' input-channel maxima, the plan of every smoothed Linear (host), the int8 weights again.
int finish_smoothing(td_flux* root, hipStream_t s) {
  const int64_t D = root->D, M = root->M, n = root->smooth_n;
  const int L = root->cfg.num_layers, Ls = root->cfg.num_single_layers;
  TD_CHECK_HIP(hipMemsetAsync(root->sm_aw, 0, (size_t)n * 4, s));
  for (int i = 0; i < L; ++i) {
    const DoubleW& w = root->dbl[i];
    unsigned* a = root->sm_aw + sm_dbl(root, i);
    TD_TRY(td_col_amax_launch(w.qkv_img_w, (int)D, (int)(3 * D), (int)D, a, s));
    TD_TRY(td_col_amax_launch(w.qkv_ctx_w, (int)D, (int)(3 * D), (int)D, a + D, s));
    TD_TRY(td_col_amax_launch(w.ff1_img_w, (int)D, (int)M, (int)D, a + 2 * D, s));
    TD_TRY(td_col_amax_launch(w.ff1_ctx_w, (int)D, (int)M, (int)D, a + 3 * D, s));
    TD_TRY(td_col_amax_launch(w.ff2_img_w, (int)M, (int)D, (int)M, a + 4 * D, s));
    TD_TRY(td_col_amax_launch(w.ff2_ctx_w, (int)M, (int)D, (int)M, a + 4 * D + M, s));
  }
  for (int i = 0; i < Ls; ++i) {
    unsigned* a = root->sm_aw + sm_sgl(root, i);
    TD_TRY(td_col_amax_launch(root->sgl[i].w1, (int)D, (int)(3 * D + M), (int)D, a, s));
    TD_TRY(td_col_amax_launch(root->sgl[i].w2, (int)(D + M), (int)D, (int)(D + M), a + D, s));
  }
  std::vector<float> ax(n), aw(n), sw(n), inv(n);
  std::vector<bf16_t> inv16(n);
  std::vector<int> ext((size_t)(4 * L + Ls) * SM_EXT, -1);
  TD_CHECK_HIP(hipMemcpyAsync(ax.data(), root->sm_ax, (size_t)n * 4, hipMemcpyDeviceToHost, s));      // (float bits of non-negative values)
  TD_CHECK_HIP(hipMemcpyAsync(aw.data(), root->sm_aw, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  TD_CHECK_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < L; ++i) {
    const int64_t o = sm_dbl(root, i);
    for (int k = 0; k < 4; ++k)      // qkv_img, qkv_ctx, ff1_img, ff1_ctx: LayerNorm-fed, replication available
      smooth_plan(&ax[o + k * D], &aw[o + k * D], (int)D, &sw[o + k * D], &inv[o + k * D], &ext[(size_t)(4 * i + k) * SM_EXT]);
    smooth_plan(&ax[o + 4 * D], &aw[o + 4 * D], (int)M, &sw[o + 4 * D], &inv[o + 4 * D], nullptr);
    smooth_plan(&ax[o + 4 * D + M], &aw[o + 4 * D + M], (int)M, &sw[o + 4 * D + M], &inv[o + 4 * D + M], nullptr);
  }
  for (int i = 0; i < Ls; ++i) {
    const int64_t o = sm_sgl(root, i);
    smooth_plan(&ax[o], &aw[o], (int)D, &sw[o], &inv[o], &ext[(size_t)(4 * L + i) * SM_EXT]);
    for (int64_t c = 0; c < D; ++c) { sw[o + D + c] = 1.f; inv[o + D + c] = 1.f; }      // w2's attention half: never smoothed
    smooth_plan(&ax[o + 2 * D], &aw[o + 2 * D], (int)M, &sw[o + 2 * D], &inv[o + 2 * D], nullptr);
  }
  for (int64_t c = 0; c < n; ++c) {      // bf16 of a power of two: its top 16 bits
    unsigned u; std::memcpy(&u, &inv[c], 4);
    inv16[c] = (bf16_t)(u >> 16);
  }
  TD_CHECK_HIP(hipMemcpyAsync(root->sm_s, sw.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(root->sm_inv, inv.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(root->sm_inv16, inv16.data(), (size_t)n * 2, hipMemcpyHostToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(root->sm_ext, ext.data(), ext.size() * sizeof(int), hipMemcpyHostToDevice, s));
  TD_CHECK_HIP(hipStreamSynchronize(s));      // the host vectors go out of scope below
  // int8 weights again: column factors, and for the LayerNorm-fed ones rows of D + SM_EXT bytes with the replicated channels behind the real ones
  auto qz = [&](const bf16_t* w, const Fp8Mat& m, int64_t rows, int64_t K, const float* col, const int* ex) -> int {
    const int ld = (int)(ex ? K + SM_EXT : K);
    TD_TRY(td_quant_rows_fp8_launch(w, (int)K, m.q, ld, m.s, (int)rows, (int)K, s, 1, nullptr, col));
    if (ex) TD_TRY(td_ext_cols_launch(m.q, ld, (int)rows, (int)K, ex, SM_EXT, s));
    return TD_OK;
  };
  for (int i = 0; i < L; ++i) {
    const DoubleW& w = root->dbl[i];
    const DoubleW8& q = root->dbl8[i];
    const float* c = root->sm_s + sm_dbl(root, i);
    const int* ex = root->sm_ext + (size_t)4 * i * SM_EXT;
    TD_TRY(qz(w.qkv_img_w, q.qkv_img, 3 * D, D, c, ex)); TD_TRY(qz(w.qkv_ctx_w, q.qkv_ctx, 3 * D, D, c + D, ex + SM_EXT));
    TD_TRY(qz(w.ff1_img_w, q.ff1_img, M, D, c + 2 * D, ex + 2 * SM_EXT)); TD_TRY(qz(w.ff1_ctx_w, q.ff1_ctx, M, D, c + 3 * D, ex + 3 * SM_EXT));
    TD_TRY(qz(w.ff2_img_w, q.ff2_img, D, M, c + 4 * D, nullptr)); TD_TRY(qz(w.ff2_ctx_w, q.ff2_ctx, D, M, c + 4 * D + M, nullptr));
  }
  for (int i = 0; i < Ls; ++i) {
    const float* c = root->sm_s + sm_sgl(root, i);
    TD_TRY(qz(root->sgl[i].w1, root->sgl8[i].w1, 3 * D + M, D, c, root->sm_ext + (size_t)(4 * L + i) * SM_EXT));
    TD_TRY(qz(root->sgl[i].w2, root->sgl8[i].w2, D, D + M, c + D, nullptr));
  }
  TD_CHECK_HIP(hipStreamSynchronize(s));      // other contexts' streams read these weights next
  root->smooth_ready = true;
  ++root->hist_epoch;                          // scales recorded under the unsmoothed form say nothing about the smoothed one
  return TD_OK;
}
}  // namespace

extern "C" {

// The joint attention of every block: TD_ATTENTION_BF16 (default, the reference graph's arithmetic) or TD_ATTENTION_FP8 -- QK^T and P.V on
// the e4m3 matrix instruction (csrc/attention_fp8.hip).  Independent of td_flux_set_precision; meant for the 8-bit modes, where the
// attention is otherwise a quarter of the image.
int td_flux_set_attention(td_flux* f, int mode) {
  TD_CHECK_ARG(f && !f->parent && (mode == TD_ATTENTION_BF16 || mode == TD_ATTENTION_FP8), "td_flux_set_attention: parent context, TD_ATTENTION_BF16 or TD_ATTENTION_FP8");
  f->attn_mode = mode;
  ++f->hist_epoch;
  return TD_OK;
}

int td_flux_set_precision(td_flux* f, int precision, void* stream) {
  TD_CHECK_ARG(f && (precision == TD_PRECISION_BF16 || precision == TD_PRECISION_FP8_E4M3 || precision == TD_PRECISION_INT8), "td_flux_set_precision: unknown precision %d", precision);
  TD_CHECK_ARG(!f->parent, "td_flux_set_precision: set the precision on the parent context (forks follow it)");
  ++f->hist_epoch;
  f->smooth_ready = false;      // the weights are quantised afresh below, unsmoothed: the next int8 forward calibrates again
  if (precision == TD_PRECISION_BF16) { f->precision = precision; return TD_OK; }
  TD_CHECK_ARG(f->D % 128 == 0 && f->M % 128 == 0, "td_flux_set_precision: fp8 needs inner widths that are multiples of 128");
  hipStream_t s = (hipStream_t)stream;
  const int64_t D = f->D, M = f->M, L = f->cfg.num_layers, Ls = f->cfg.num_single_layers;
  if (!f->arena8) {
    auto al = [](int64_t b) { return (b + 255) & ~int64_t(255); };
    const int64_t DE = D + SM_EXT;      // LayerNorm-fed Linears: room for the replicated input channels of the smoothed form
    const int64_t per_double = 2 * (al(3 * D * DE) + al(D * D) + al(M * DE) + al(D * M)) + 2 * (al(3 * D * 4) + al(D * 4) + al(M * 4) + al(D * 4));
    const int64_t per_single = al((3 * D + M) * DE) + al(D * (D + M)) + al((3 * D + M) * 4) + al(D * 4);
    const int64_t total = L * per_double + Ls * per_single;
    hipError_t e = hipMalloc((void**)&f->arena8, (size_t)total);
    if (e != hipSuccess) {
      td_set_error("td_flux_set_precision: hipMalloc of %.2f GiB fp8 arena failed: %s", total / double(1 << 30), hipGetErrorString(e));
      return TD_ERR_HIP;
    }
    int64_t o = 0;
    auto take = [&](int64_t rows, int64_t K) {
      Fp8Mat m;
      m.q = (uint8_t*)(f->arena8 + o); o += al(rows * K);
      m.s = (float*)(f->arena8 + o); o += al(rows * 4);
      return m;
    };
    f->dbl8.resize(L);
    f->sgl8.resize(Ls);
    for (auto& w : f->dbl8) {
      w.qkv_img = take(3 * D, DE); w.qkv_ctx = take(3 * D, DE); w.out_img = take(D, D); w.out_ctx = take(D, D);
      w.ff1_img = take(M, DE); w.ff1_ctx = take(M, DE); w.ff2_img = take(D, M); w.ff2_ctx = take(D, M);
    }
    for (auto& w : f->sgl8) { w.w1 = take(3 * D + M, DE); w.w2 = take(D, D + M); }
  }
  auto qz = [&](const bf16_t* w, const Fp8Mat& m, int64_t rows, int64_t K) {
    return td_quant_rows_fp8_launch(w, (int)K, m.q, (int)K, m.s, (int)rows, (int)K, s, precision == TD_PRECISION_INT8);
  };
  for (int i = 0; i < L; ++i) {
    const DoubleW& w = f->dbl[i];
    const DoubleW8& q = f->dbl8[i];
    TD_TRY(qz(w.qkv_img_w, q.qkv_img, 3 * D, D)); TD_TRY(qz(w.qkv_ctx_w, q.qkv_ctx, 3 * D, D));
    TD_TRY(qz(w.out_img_w, q.out_img, D, D)); TD_TRY(qz(w.out_ctx_w, q.out_ctx, D, D));
    TD_TRY(qz(w.ff1_img_w, q.ff1_img, M, D)); TD_TRY(qz(w.ff1_ctx_w, q.ff1_ctx, M, D));
    TD_TRY(qz(w.ff2_img_w, q.ff2_img, D, M)); TD_TRY(qz(w.ff2_ctx_w, q.ff2_ctx, D, M));
  }
  for (int i = 0; i < Ls; ++i) {
    TD_TRY(qz(f->sgl[i].w1, f->sgl8[i].w1, 3 * D + M, D));
    TD_TRY(qz(f->sgl[i].w2, f->sgl8[i].w2, D, D + M));
  }
  f->precision = precision;
  return TD_OK;
}

}  // extern "C"

// ---- LoRA adapter registry ---------------------------------------------------------------------------------------------------------------------
namespace {

int lora_find(const LoraState* ls, const char* name) {
  if (ls) for (size_t i = 0; i < ls->adapters.size(); ++i) if (ls->adapters[i].name == name) return (int)i;
  return -1;
}

// the pairs that act on `slot` under the current active set, in adapter order; false: more than one merge launch takes
bool lora_active_on(const LoraState* ls, int slot, std::vector<const void*>* packed, std::vector<int>* ranks, std::vector<float>* scales) {
  int n = 0;
  for (const LoraAdapter& a : ls->adapters) {
    if (!a.active || a.weight == 0.f) continue;
    for (const LoraPair& p : a.pairs) {
      if (p.slot != slot) continue;
      if (++n > TD_LORA_MAX_ADAPTERS) return false;
      if (packed) { packed->push_back(p.packed); ranks->push_back(p.rank); scales->push_back(a.weight * p.scale); }
    }
  }
  return true;
}

// Recompute the arena's copy of every slot in `slots` from its base copy, free the base copies no pair needs any more, then everything a weight
// change entails: weight epoch, 8-bit history / smoothing calibration, the 8-bit weights themselves.
int lora_remerge(td_flux* f, const std::vector<int>& slots, hipStream_t s) {
  LoraState* ls = f->lora;
  for (int slot : slots)
    TD_CHECK_ARG(lora_active_on(ls, slot, nullptr, nullptr, nullptr), "td_flux_lora: more than %d active adapters on '%s'", TD_LORA_MAX_ADAPTERS,
                 f->slots[slot].name.c_str());
  auto touched = [&](int slot) {
    for (const LoraAdapter& a : ls->adapters) for (const LoraPair& p : a.pairs) if (p.slot == slot) return true;
    return false;
  };
  bool orphans = false;
  for (int slot : slots) {
    auto it = ls->base.find(slot);
    if (it == ls->base.end()) continue;
    const Slot& sl = f->slots[slot];
    std::vector<const void*> packed; std::vector<int> ranks; std::vector<float> scales;
    lora_active_on(ls, slot, &packed, &ranks, &scales);
    TD_TRY(td_lora_merge_bf16(it->second, sl.ptr, (int)sl.rows, (int)sl.cols, (int)packed.size(), packed.data(), ranks.data(), scales.data(), s));
    orphans |= !touched(slot);
  }
  if (orphans) {      // base copies no pair needs any more: their bits are back in the arena once the stream has drained
    TD_CHECK_HIP(hipStreamSynchronize(s));
    for (int slot : slots) {
      auto it = ls->base.find(slot);
      if (it != ls->base.end() && !touched(slot)) { (void)hipFree(it->second); ls->base.erase(it); }
    }
  }
  ++f->weight_epoch;
  ++f->hist_epoch;
  f->smooth_ready = false;
  if (f->precision != TD_PRECISION_BF16) TD_TRY(td_flux_set_precision(f, f->precision, s));      // the 8-bit weights again, from the merged ones
  return TD_OK;
}

std::vector<int> lora_all_slots(const LoraState* ls) {
  std::vector<int> v;
  for (const auto& b : ls->base) v.push_back(b.first);
  std::sort(v.begin(), v.end());
  return v;
}

}  // namespace

extern "C" {

int td_flux_read_param(td_flux* f, const char* name, void* dst, int64_t count, void* stream) {
  TD_CHECK_ARG(f && name && dst, "td_flux_read_param: null argument");
  auto it = f->index.find(name);
  TD_CHECK_ARG(it != f->index.end(), "td_flux_read_param: unknown parameter '%s'", name);
  const Slot& s = f->slots[it->second];
  TD_CHECK_ARG(s.count == count, "td_flux_read_param: '%s' holds %lld elements, the destination %lld", name, (long long)s.count, (long long)count);
  TD_CHECK_HIP(hipMemcpyAsync(dst, s.ptr, (size_t)count * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

int td_flux_param_shape(const td_flux* f, const char* name, int64_t* rows, int64_t* cols) {
  TD_CHECK_ARG(f && name, "td_flux_param_shape: null argument");
  auto it = f->index.find(name);
  TD_CHECK_ARG(it != f->index.end(), "td_flux_param_shape: unknown parameter '%s'", name);
  if (rows) *rows = f->slots[it->second].rows;
  if (cols) *cols = f->slots[it->second].cols;
  return TD_OK;
}

int td_flux_lora_load(td_flux* f, const char* adapter, const char* param, const void* A, const void* B, int rank, float scale, void* stream) {
  TD_CHECK_ARG(f && adapter && param && A && B, "td_flux_lora_load: null argument");
  TD_CHECK_ARG(!f->parent, "td_flux_lora_load: '%s': adapters belong to the parent context (forks see its weights)", param);
  TD_CHECK_ARG(adapter[0], "td_flux_lora_load: empty adapter name");
  auto it = f->index.find(param);
  TD_CHECK_ARG(it != f->index.end(), "td_flux_lora_load: unknown parameter '%s'", param);
  const int slot = it->second;
  const Slot& sl = f->slots[slot];
  const size_t pl = strlen(param);
  TD_CHECK_ARG(sl.cols > 1 && pl > 7 && strcmp(param + pl - 7, ".weight") == 0, "td_flux_lora_load: '%s' is not the weight of a Linear (%lld elements, 1-D): "
               "bias and norm-scale deltas are not built", param, (long long)sl.count);
  TD_CHECK_ARG(rank >= 1, "td_flux_lora_load: '%s': rank=%d must be at least 1", param, rank);
  TD_CHECK_ARG(std::isfinite(scale), "td_flux_lora_load: '%s': scale is not finite", param);
  TD_CHECK_ARG((uintptr_t)A % 16 == 0 && (uintptr_t)B % 16 == 0, "td_flux_lora_load: '%s': A and B must be 16-byte aligned", param);
  TD_CHECK_ARG(sl.cols % 64 == 0 && sl.rows % 8 == 0 && sl.rows < (1ll << 31) && sl.cols < (1ll << 31), "td_flux_lora_load: '%s' is [%lld, %lld]: the merge "
               "needs rows %% 8 == 0 and columns %% 64 == 0", param, (long long)sl.rows, (long long)sl.cols);
  if (!f->lora) f->lora = new LoraState();
  LoraState* ls = f->lora;
  int ai = lora_find(ls, adapter);
  if (ai >= 0)
    for (const LoraPair& p : ls->adapters[ai].pairs)
      TD_CHECK_ARG(p.slot != slot, "td_flux_lora_load: adapter '%s' already holds a pair for '%s'", adapter, param);
  hipStream_t s = (hipStream_t)stream;
  LoraPair p;
  p.slot = slot; p.rank = rank; p.scale = scale;
  p.bytes = (int64_t)td_lora_packed_bytes(rank, (int)sl.rows, (int)sl.cols);
  hipError_t e = hipMalloc((void**)&p.packed, (size_t)p.bytes);
  if (e != hipSuccess) { td_set_error("td_flux_lora_load: '%s': hipMalloc of %lld operand bytes failed: %s", param, (long long)p.bytes, hipGetErrorString(e)); return TD_ERR_HIP; }
  if (int rc = td_lora_pack_bf16(A, B, rank, (int)sl.rows, (int)sl.cols, p.packed, s)) { (void)hipFree(p.packed); return rc; }
  if (!ls->base.count(slot)) {
    bf16_t* base = nullptr;
    e = hipMalloc((void**)&base, (size_t)sl.count * 2);
    if (e == hipSuccess) e = hipMemcpyAsync(base, sl.ptr, (size_t)sl.count * 2, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      td_set_error("td_flux_lora_load: '%s': base copy of %lld bytes failed: %s", param, (long long)sl.count * 2, hipGetErrorString(e));
      (void)hipStreamSynchronize(s);
      (void)hipFree(p.packed); if (base) (void)hipFree(base);
      return TD_ERR_HIP;
    }
    ls->base[slot] = base;
  }
  if (ai < 0) { ls->adapters.emplace_back(); ls->adapters.back().name = adapter; ai = (int)ls->adapters.size() - 1; }
  ls->adapters[ai].pairs.push_back(p);
  return TD_OK;
}

int td_flux_lora_set_adapters(td_flux* f, const char* const* names, const float* weights, int n, void* stream) {
  TD_CHECK_ARG(f && n >= 0 && (n == 0 || (names && weights)), "td_flux_lora_set_adapters: null argument");
  TD_CHECK_ARG(!f->parent, "td_flux_lora_set_adapters: adapters belong to the parent context (forks see its weights)");
  LoraState* ls = f->lora;
  std::vector<int> idx(n);
  for (int i = 0; i < n; ++i) {
    TD_CHECK_ARG(names[i], "td_flux_lora_set_adapters: name %d is null", i);
    idx[i] = lora_find(ls, names[i]);
    TD_CHECK_ARG(idx[i] >= 0, "td_flux_lora_set_adapters: unknown adapter '%s'", names[i]);
    TD_CHECK_ARG(std::isfinite(weights[i]), "td_flux_lora_set_adapters: the weight of adapter '%s' is not finite", names[i]);
    for (int j = 0; j < i; ++j) TD_CHECK_ARG(idx[j] != idx[i], "td_flux_lora_set_adapters: adapter '%s' is named twice", names[i]);
  }
  if (!ls) return TD_OK;      // nothing loaded, nothing named
  std::vector<std::pair<bool, float>> before;
  for (LoraAdapter& a : ls->adapters) { before.emplace_back(a.active, a.weight); a.active = false; a.weight = 0.f; }
  for (int i = 0; i < n; ++i) { ls->adapters[idx[i]].active = true; ls->adapters[idx[i]].weight = weights[i]; }
  const std::vector<int> slots = lora_all_slots(ls);
  for (int slot : slots)
    if (!lora_active_on(ls, slot, nullptr, nullptr, nullptr)) {      // refused: nothing changes
      for (size_t i = 0; i < before.size(); ++i) { ls->adapters[i].active = before[i].first; ls->adapters[i].weight = before[i].second; }
      td_set_error("td_flux_lora_set_adapters: more than %d active adapters on '%s'", TD_LORA_MAX_ADAPTERS, f->slots[slot].name.c_str());
      return TD_ERR_INVALID;
    }
  return lora_remerge(f, slots, (hipStream_t)stream);
}

int td_flux_lora_delete(td_flux* f, const char* adapter, void* stream) {
  TD_CHECK_ARG(f && adapter, "td_flux_lora_delete: null argument");
  TD_CHECK_ARG(!f->parent, "td_flux_lora_delete: adapters belong to the parent context (forks see its weights)");
  const int ai = lora_find(f->lora, adapter);
  TD_CHECK_ARG(ai >= 0, "td_flux_lora_delete: unknown adapter '%s'", adapter);
  LoraState* ls = f->lora;
  TD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));      // its operands may still be read by a merge in flight
  std::vector<int> slots;
  for (LoraPair& p : ls->adapters[ai].pairs) { slots.push_back(p.slot); (void)hipFree(p.packed); }
  ls->adapters.erase(ls->adapters.begin() + ai);
  return lora_remerge(f, slots, (hipStream_t)stream);
}

int td_flux_lora_clear(td_flux* f, void* stream) {
  TD_CHECK_ARG(f, "td_flux_lora_clear: null handle");
  TD_CHECK_ARG(!f->parent, "td_flux_lora_clear: adapters belong to the parent context (forks see its weights)");
  LoraState* ls = f->lora;
  if (!ls || (ls->adapters.empty() && ls->base.empty())) return TD_OK;
  TD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (LoraAdapter& a : ls->adapters) for (LoraPair& p : a.pairs) (void)hipFree(p.packed);
  ls->adapters.clear();
  return lora_remerge(f, lora_all_slots(ls), (hipStream_t)stream);
}

int td_flux_lora_info(const td_flux* f, int* n_adapters, int* n_params_touched, int64_t* bytes_held) {
  TD_CHECK_ARG(f, "td_flux_lora_info: null handle");
  const LoraState* ls = (f->parent ? f->parent : f)->lora;
  int64_t bytes = 0;
  if (ls) {
    for (const LoraAdapter& a : ls->adapters) for (const LoraPair& p : a.pairs) bytes += p.bytes;
    for (const auto& b : ls->base) bytes += f->slots[b.first].count * 2;
  }
  if (n_adapters) *n_adapters = ls ? (int)ls->adapters.size() : 0;
  if (n_params_touched) *n_params_touched = ls ? (int)ls->base.size() : 0;
  if (bytes_held) *bytes_held = bytes;
  return TD_OK;
}

}  // extern "C"

struct FloatPack { static constexpr int N = 128; float v[N]; };
__global__ void td_set_floats_kernel(float* dst, FloatPack vals, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}

// ---- synthetic checkpoint: counter-based N(0, std) (full-shape random init for throughput runs) ------
// Grid-stride: a launch carries at most 2^32 - 1 work-items (the dispatch packet's grid size is 32 bits and a larger product is
// truncated WITHOUT an error) -- the 11.9 B-parameter FLUX arena needs 5.95 G pairs.  The one-thread-per-pair form filled only
// the first 3.3 G elements of it (embedders + modulation matrix) and left every block weight at the allocator's zeros.
__global__ void td_fill_normal_kernel(bf16_t* dst, long long n, unsigned long long seed, float std, float mean) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long pair = (long long)blockIdx.x * blockDim.x + threadIdx.x; 2 * pair < n; pair += stride) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(pair + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    const float u1 = ((unsigned)(z >> 40) + 1.0f) * (1.0f / 16777217.0f);
    const float u2 = (unsigned)((z >> 8) & 0xffffff) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.283185307179586f * u2, &s, &c);
    dst[2 * pair] = f2bf(mean + std * r * c);
    if (2 * pair + 1 < n) dst[2 * pair + 1] = f2bf(mean + std * r * s);
  }
}

extern "C" {

int td_fill_normal_bf16(void* dst, int64_t n, uint64_t seed, float std, float mean, void* stream) {
  TD_CHECK_ARG(dst && n > 0, "td_fill_normal_bf16: empty buffer");
  const long long pairs = (n + 1) / 2;
  const long long blocks = (pairs + 255) / 256;
  hipLaunchKernelGGL(td_fill_normal_kernel, dim3((unsigned)(blocks < (1ll << 20) ? blocks : (1ll << 20))), dim3(256), 0, (hipStream_t)stream,
                     (bf16_t*)dst, (long long)n, (unsigned long long)seed, std, mean);
  TD_CHECK_LAUNCH();
  return TD_OK;
}

int td_flux_init_random(td_flux* f, uint64_t seed, float std, void* stream) {
  TD_CHECK_ARG(f, "td_flux_init_random: null handle");
  {
    const LoraState* ls = (f->parent ? f->parent : f)->lora;
    TD_CHECK_ARG(!ls || ls->base.empty(), "td_flux_init_random: %d parameters carry LoRA adapters (their base copies would go stale): clear the adapters first "
                 "(td_flux_lora_clear)", ls ? (int)ls->base.size() : 0);
  }
  (f->parent ? f->parent : f)->bounds_dirty = true;
  ++(f->parent ? f->parent : f)->hist_epoch;
  (f->parent ? f->parent : f)->smooth_ready = false;
  TD_TRY(td_fill_normal_bf16(f->arena, f->arena_elems, seed, std, 0.f, stream));
  for (const Slot& s : f->slots)
    if (s.count == 128 && s.name.find(".norm_") != std::string::npos)
      TD_TRY(td_fill_normal_bf16(s.ptr, s.count, seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(s.ptr - f->arena + 1)), 0.1f, 1.0f, stream));
  return TD_OK;
}

// Conditioning of one prompt: context_embedder(prompt_embeds), text_embedder(pooled), RoPE tables.
// img_ids/txt_ids are device fp32 [n,3]; txt_ids NULL = zeros (thinkdiff/models/flux_prompt.py:119).
int td_flux_set_condition(td_flux* f, const void* prompt_embeds, int T, const void* pooled, const float* txt_ids,
                          const float* img_ids, int S_img, void* stream) {
  TD_CHECK_ARG(f && prompt_embeds && pooled && img_ids, "td_flux_set_condition: null argument");
  TD_CHECK_ARG(T > 0 && T <= f->max_txt && S_img > 0 && S_img <= f->max_img,
               "td_flux_set_condition: T=%d / S_img=%d exceed capacity (%d / %d)", T, S_img, f->max_txt, f->max_img);
  hipStream_t s = (hipStream_t)stream;
  const int D = f->D;
  if (S_img != f->S_img) f->ccond_set = false;      // the channel condition was written for another token count
  f->T = T; f->S_img = S_img;
  f->S_ref = 0;      // the tables below hold T + S_img rows: reference tokens are set again after the condition, for every image
  TD_TRY(gemm(f, s, (const bf16_t*)prompt_embeds, f->cfg.joint_dim, f->ctx_w, f->ctx_b, f->ctx, D, T, D, f->cfg.joint_dim));
  TD_TRY(gemm(f, s, (const bf16_t*)pooled, f->cfg.pooled_dim, f->p1_w, f->p1_b, f->pmid, D, 1, D, f->cfg.pooled_dim, TD_ACT_SILU));
  TD_TRY(gemm(f, s, f->pmid, D, f->p2_w, f->p2_b, f->pe, D, 1, D, D));
  if (txt_ids) TD_CHECK_HIP(hipMemcpyAsync(f->ids, txt_ids, (size_t)T * 12, hipMemcpyDeviceToDevice, s));
  else TD_CHECK_HIP(hipMemsetAsync(f->ids, 0, (size_t)T * 12, s));
  TD_CHECK_HIP(hipMemcpyAsync(f->ids + (size_t)T * 3, img_ids, (size_t)S_img * 12, hipMemcpyDeviceToDevice, s));
  TD_TRY(td_flux_rope_table_launch(f->ids, T + S_img, f->cfg.axes_dims, (double)f->cfg.rope_theta, f->cosT, f->sinT, s));
  f->cond_set = true;
  f->cond_epoch = (f->parent ? f->parent : f)->weight_epoch;
  f->n_steps = 0;
  f->hs_step = f->href_step = -1;      // another image: the previous one's maxima / reference points say nothing about it
  return TD_OK;
}

// The channel condition of one image (conditioned engines): cond [S_img, Ccond] -> xin[:, Cout .. Cin), where every forward's x_embedder
// GEMM reads it beside the gathered latents.
int td_flux_set_channel_condition(td_flux* f, const void* cond, void* stream) {
  TD_CHECK_ARG(f && cond, "td_flux_set_channel_condition: null argument");
  TD_CHECK_ARG(f->Ccond > 0, "td_flux_set_channel_condition: this engine takes no channel condition (in_channels = out_channels = %d)", f->Cout);
  TD_CHECK_ARG(f->cond_set, "td_flux_set_channel_condition: call td_flux_set_condition first (it fixes the image token count)");
  TD_CHECK_ARG((uintptr_t)cond % 16 == 0, "td_flux_set_channel_condition: cond must be 16-byte aligned");
  TD_TRY(td_copy_cols_launch((const bf16_t*)cond, f->Ccond, f->xin + f->Cout, f->Cin, f->S_img, f->Ccond, (hipStream_t)stream));
  f->ccond_set = true;
  f->hs_step = f->href_step = -1;      // another image, as in td_flux_set_condition: the previous one's per-token history says nothing about it
  return TD_OK;
}

// The reference tokens of one image (FLUX.1 Kontext): [ext] diffusers >= 0.34 FluxKontextPipeline.__call__
//   latent_model_input = torch.cat([latents, image_latents], dim=1);  latent_ids = torch.cat([latent_ids, image_ids], dim=0)
// ref_latents [S_ref, Cout] -> xref rows S_img ..; ref_ids [S_ref, 3] -> rows T + S_img .. of the id / RoPE tables (td_flux_rope_table's arithmetic).
int td_flux_set_reference_tokens(td_flux* f, const void* ref_latents, int S_ref, const float* ref_ids, void* stream) {
  TD_CHECK_ARG(f, "td_flux_set_reference_tokens: null context");
  TD_CHECK_ARG(S_ref >= 0, "td_flux_set_reference_tokens: S_ref=%d is negative", S_ref);
  TD_CHECK_ARG(f->Ccond == 0, "td_flux_set_reference_tokens: this engine is channel-conditioned (in_channels=%d, out_channels=%d); reference tokens "
               "belong to the unconditioned FLUX.1 Kontext transformer", f->Cin, f->Cout);
  TD_CHECK_ARG(f->cond_set, "td_flux_set_reference_tokens: call td_flux_set_condition first (it fixes the text and image token counts; S_ref=%d)", S_ref);
  if (S_ref == 0) {
    f->S_ref = 0;
    f->hs_step = f->href_step = -1;
    return TD_OK;
  }
  TD_CHECK_ARG(ref_latents && ref_ids, "td_flux_set_reference_tokens: null ref_latents / ref_ids with S_ref=%d", S_ref);
  TD_CHECK_ARG((long long)f->S_img + S_ref <= f->max_img, "td_flux_set_reference_tokens: S_img=%d + S_ref=%d exceed the image-stream capacity %d "
               "(max_img_tokens of td_flux_create)", f->S_img, S_ref, f->max_img);
  TD_CHECK_ARG((uintptr_t)ref_latents % 16 == 0 && (uintptr_t)ref_ids % 4 == 0, "td_flux_set_reference_tokens: ref_latents must be 16-byte, ref_ids 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const size_t row0 = (size_t)f->T + f->S_img;
  TD_CHECK_HIP(hipMemcpyAsync(f->xref + (size_t)f->S_img * f->Cout, ref_latents, (size_t)S_ref * f->Cout * 2, hipMemcpyDeviceToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(f->ids + row0 * 3, ref_ids, (size_t)S_ref * 12, hipMemcpyDeviceToDevice, s));
  TD_TRY(td_flux_rope_table_launch(f->ids + row0 * 3, S_ref, f->cfg.axes_dims, (double)f->cfg.rope_theta, f->cosT + row0 * 128, f->sinT + row0 * 128, s));
  f->S_ref = S_ref;
  f->hs_step = f->href_step = -1;      // another image, as in td_flux_set_condition: the previous one's per-token history says nothing about it
  return TD_OK;
}

int td_flux_reference_tokens(const td_flux* f, int* S_ref) {
  TD_CHECK_ARG(f && S_ref, "td_flux_reference_tokens: null argument");
  *S_ref = f->cond_set ? f->S_ref : 0;
  return TD_OK;
}

// temb and ALL adaLN modulations for the whole schedule.  t_eff[i] / g_eff are the scalars the
// sinusoids see (timestep*1000 and guidance*1000 after the caller's dtype handling); host pointers.
int td_flux_set_timesteps(td_flux* f, const float* t_eff, int n, float g_eff, void* stream) {
  TD_CHECK_ARG(f && t_eff && n > 0 && n <= f->max_steps, "td_flux_set_timesteps: n=%d exceeds capacity %d", n, f ? f->max_steps : 0);
  TD_CHECK_ARG(f->cond_set, "td_flux_set_timesteps: call td_flux_set_condition first (temb includes the pooled text embedding)");
  {
    td_flux* root = f->parent ? f->parent : f;
    if (root->bounds_dirty) TD_TRY(refresh_score_bounds(root));      // (once per weight change; set_timesteps calls are serial on the host)
  }
  hipStream_t s = (hipStream_t)stream;
  const int D = f->D;
  // The schedule scalars travel BY VALUE in a kernel argument (stream-ordered, no host buffer whose lifetime or reallocation
  // could race a deferred copy); schedules longer than the pack take a synchronous copy instead.
  if (n + 1 <= FloatPack::N) {
    FloatPack fp;
    for (int i = 0; i < n; ++i) fp.v[i] = t_eff[i];
    fp.v[n] = g_eff;
    hipLaunchKernelGGL(td_set_floats_kernel, dim3(1), dim3(FloatPack::N), 0, s, f->tvals, fp, n + 1);
    TD_CHECK_LAUNCH();
  } else {
    f->tv_host.assign(t_eff, t_eff + n);
    f->tv_host.push_back(g_eff);
    TD_CHECK_HIP(hipMemcpyAsync(f->tvals, f->tv_host.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, s));
    TD_CHECK_HIP(hipStreamSynchronize(s));
  }
  TD_TRY(td_timestep_sincos_launch(f->tvals, n, f->tproj, s));
  TD_TRY(gemm(f, s, f->tproj, 256, f->t1_w, f->t1_b, f->tmid, D, n, D, 256, TD_ACT_SILU));
  TD_TRY(gemm(f, s, f->tmid, D, f->t2_w, f->t2_b, f->te, D, n, D, D));
  if (f->cfg.guidance_embeds) {
    TD_TRY(td_timestep_sincos_launch(f->tvals + n, 1, f->gproj, s));
    TD_TRY(gemm(f, s, f->gproj, 256, f->g1_w, f->g1_b, f->gmid, D, 1, D, 256, TD_ACT_SILU));
    TD_TRY(gemm(f, s, f->gmid, D, f->g2_w, f->g2_b, f->ge, D, 1, D, D));
  }
  TD_TRY(td_temb_combine_silu_launch(f->te, f->cfg.guidance_embeds ? f->ge : nullptr, f->pe, n, D, f->temb, f->st, s));
  TD_TRY(gemm_big_n(f, s, f->st, D, f->mod_w, f->mod_b, f->mods, f->NMOD, n, f->NMOD, D));
  f->n_steps = n;
  f->sched_epoch = (f->parent ? f->parent : f)->weight_epoch;
  f->hs_step = f->href_step = -1;      // another schedule: "the previous step" of the old one is not this one's
  return TD_OK;
}

// One transformer evaluation: velocity[S_img, out_channels] = FluxTransformer2DModel(latents; step).
// What the prepared context expects of its callers' buffers (the torch.ops layer validates tensor extents against it).
int td_flux_prepared_shape(const td_flux* f, int* img_tokens, int* txt_tokens, int* in_channels, int* n_steps) {
  TD_CHECK_ARG(f, "td_flux_prepared_shape: null context");
  if (img_tokens) *img_tokens = f->cond_set ? f->S_img : 0;
  if (txt_tokens) *txt_tokens = f->cond_set ? f->T : 0;
  if (in_channels) *in_channels = f->Cout;      // the latents' and the velocity's width (== x_embedder's on an unconditioned engine)
  if (n_steps) *n_steps = f->n_steps;
  return TD_OK;
}

int td_flux_input_shape(const td_flux* f, int* in_channels, int* cond_channels, int* cond_valid) {
  TD_CHECK_ARG(f, "td_flux_input_shape: null context");
  if (in_channels) *in_channels = f->Cin;
  if (cond_channels) *cond_channels = f->Ccond;
  if (cond_valid) *cond_valid = f->Ccond > 0 && f->cond_set && f->ccond_set;
  return TD_OK;
}

int td_flux_forward(td_flux* f, const void* latents, int step, void* velocity, void* stream) {
  TD_CHECK_ARG(f && latents && velocity, "td_flux_forward: null argument");
  TD_CHECK_ARG(f->cond_set && step >= 0 && step < f->n_steps, "td_flux_forward: step %d outside the %d prepared timesteps", step, f ? f->n_steps : 0);
  {
    const int we = (f->parent ? f->parent : f)->weight_epoch;
    TD_CHECK_ARG(f->cond_epoch == we && f->sched_epoch == we, "td_flux_forward: weights changed since td_flux_set_condition / td_flux_set_timesteps (LoRA adapters "
                 "were set, deleted or cleared; both precompute values from weights): call them again on this context");
  }
  TD_CHECK_ARG(f->Ccond == 0 || f->ccond_set, "td_flux_forward: this engine reads a %d-channel condition beside the %d latent channels and none is set for "
               "the %d image tokens (td_flux_set_channel_condition after td_flux_set_condition)", f->Ccond, f->Cout, f->S_img);
  hipStream_t s = (hipStream_t)stream;
  // Si: rows of the image stream the blocks run over (latents, then the reference tokens if any); So: the rows that are a velocity
  const int D = f->D, M = f->M, T = f->T, So = f->S_img, Si = f->S_img + f->S_ref, S = f->T + Si;
  const int H = f->cfg.num_heads, C = f->Cout;
  const int L = f->cfg.num_layers, Ls = f->cfg.num_single_layers;
  const bf16_t* mod = f->mods + (size_t)step * f->NMOD;
  bf16_t* h = f->h;
  bf16_t* h_img = h + (size_t)T * D;
  const float scale = 0.08838834764831845f;  // 128^-0.5

  TD_CHECK_HIP(hipMemcpyAsync(h, f->ctx, (size_t)T * D * 2, hipMemcpyDeviceToDevice, s));
  if (f->Ccond > 0) {      // Linear(cat(latents, cond)): the latents join the condition in xin, then ONE GEMM over K = Cin (one fp32 sum, one rounding)
    TD_CHECK_ARG((uintptr_t)latents % 16 == 0, "td_flux_forward: latents must be 16-byte aligned");
    TD_TRY(td_copy_cols_launch((const bf16_t*)latents, C, f->xin, f->Cin, Si, C, s));
    TD_TRY(gemm(f, s, f->xin, f->Cin, f->x_w, f->x_b, h_img, D, Si, D, f->Cin));
  } else if (f->S_ref > 0) {      // Linear(cat([latents, ref], dim=0)): the latents join the reference rows in xref, then ONE GEMM over all rows
    TD_CHECK_HIP(hipMemcpyAsync(f->xref, latents, (size_t)So * C * 2, hipMemcpyDeviceToDevice, s));
    TD_TRY(gemm(f, s, f->xref, C, f->x_w, f->x_b, h_img, D, Si, D, C));
  } else {
    TD_TRY(gemm(f, s, (const bf16_t*)latents, C, f->x_w, f->x_b, h_img, D, Si, D, C));
  }

  TdNormParams np;
  np.x = h; np.ldx = D; np.y = f->xn; np.ldy = D; np.rows = S; np.D = D; np.eps = 1e-6f; np.split = T;
  TdQkRopeParams rp;
  rp.qkv = f->qkv; rp.ld = 3 * D; rp.rows = S; rp.Hq = H; rp.Hk = H; rp.q_col = 0; rp.k_col = D;
  rp.cos = f->cosT; rp.sin = f->sinT; rp.split = T; rp.eps = 1e-6f;
  rp.q_premul = scale * 1.4426950408889634f;      // q leaves RoPE in the exp2 domain of the attention kernel (one bf16 rounding, as before)
  TdAttnParams ap;
  ap.Q = f->qkv; ap.K = f->qkv + D; ap.V = f->qkv + 2 * D; ap.ldq = ap.ldkv = 3 * D;
  static const int attn_tune = getenv("TD_ATTN_TUNE") ? (int)strtol(getenv("TD_ATTN_TUNE"), nullptr, 0) & ~0xff : 0;   // A/B switches of the attention kernel (experiments)
  ap.Sq = ap.Skv = S; ap.Hq = ap.Hkv = H; ap.scale = scale; ap.batch = 1; ap.sk_ws = f->attn_ws; ap.variant = f->attn_variant | attn_tune;
  ap.q_prescaled = 1;

  // fp8 mode: the LayerNorm-modulate kernel emits e4m3 rows + per-token scales directly; attention / MLP outputs
  // get a per-token quantisation pass; every block GEMM then runs on the fp8 MFMA path.
  const td_flux* root = f->parent ? f->parent : f;   // weights and precision live in the parent context
  // int8 smoothing (td_flux_set_smoothing): the first forward after a change calibrates -- it runs on the bf16 path and collects channel maxima
  td_flux* const wroot = f->parent ? f->parent : f;
  const bool sm_mode = root->precision == TD_PRECISION_INT8 && root->smooth_mode == 1;
  const bool calib = sm_mode && !root->smooth_ready;
  const bool sm_on = sm_mode && root->smooth_ready;
  if (calib) TD_CHECK_HIP(hipMemsetAsync(wroot->sm_ax, 0, (size_t)root->smooth_n * 4, s));
  const unsigned m8 = (root->precision != TD_PRECISION_BF16 && !calib) ? root->fp8_mask : 0u;      // per Linear class (8-bit operand modes)
  // 8-bit attention: its pack pass reads the raw projections and applies QK-norm + RoPE itself (bit-identical, one HBM round trip less)
  // A/B switches are read per call (tests flip them inside one process); three getenv per forward are noise next to ~600 launches
  const bool rope_in_pack = root->attn_mode == TD_ATTENTION_FP8 && getenv("TD_ATTN8_NO_FUSE") == nullptr;      // (the switch: A/B timing and the bit-identity test)
  // 8-bit attention: every row's softmax starts from the reference its largest score of the PREVIOUS step gives (and leaves this step's for the next);
  // first steps, out-of-order steps and changed token layouts start from the first tile, as the stand-alone entry point does.  TD_ATTN8_NO_HREF: A/B.
  const bool href_on = root->attn_mode == TD_ATTENTION_FP8 && getenv("TD_ATTN8_NO_HREF") == nullptr;
  const bool href_read = href_on && step > 0 && f->href_step == step - 1 && f->href_T == T && f->href_S == S && f->href_epoch == root->hist_epoch;
  const size_t href_blk = (size_t)H * S;
  int* const href_out = href_on ? f->href[f->href_cur ^ 1] : nullptr;
  const int* const href_in = href_read ? f->href[f->href_cur] : nullptr;
  // (href_out is cleared to 0x80808080 -- far below any reference -- block by block by the pack pass of each attention launch)
  // bf16 attention: the block's score bound as the softmax's fixed reference point (no row maxima, no rescales); TD_ATTN_NO_BOUND: the running-maximum form (A/B)
  const bool use_bound = root->attn_mode == TD_ATTENTION_BF16 && !root->bounds_dirty && getenv("TD_ATTN_NO_BOUND") == nullptr;
  const int q_int8 = root->precision == TD_PRECISION_INT8;
  // the LayerNorm ahead of an fp8 Linear writes e4m3 rows + scales, ahead of a bf16 one the bf16 rows
  // history scales (int8): this step quantises the MLP operands under the scales the previous step's maxima give
  const int nT = 2 * L + Ls;
  const bool hist_mode = q_int8 && root->act_scale_mode == 1 && !calib;
  const bool use_hist = hist_mode && step > 0 && f->hs_step == step - 1 && f->hs_T == T && f->hs_S == S && f->hs_epoch == root->hist_epoch;
  if (hist_mode) {
    if (use_hist) TD_TRY(td_q8_scales_from_amax_launch(f->hs_amax, f->hs_scale, f->hs_inv, (long long)nT * f->hs_cap, 1.25f, s));
    else TD_CHECK_HIP(hipMemsetAsync(f->hs_amax, 0, (size_t)nT * f->hs_cap * 4, s));
  }
  // Smoothed form: the quantised LayerNorm rows and the Linears they feed carry SM_EXT replicated channels behind the D real ones
  const int DX = sm_on ? D + SM_EXT : D;
  auto norm_for = [&](bool fp8, const bf16_t* smA = nullptr, const bf16_t* smB = nullptr, const int* exA = nullptr, const int* exB = nullptr) {
    if (fp8) { np.q = f->xq; np.ldq = DX; np.q_scale = f->xs; np.q_int8 = q_int8; } else { np.q = nullptr; np.q_scale = nullptr; }
    const bool sm = fp8 && sm_on;
    np.smoothA = sm ? smA : nullptr; np.smoothB = sm ? smB : nullptr;
    np.extA = sm ? exA : nullptr; np.extB = sm ? exB : nullptr; np.ext_n = sm ? SM_EXT : 0;
  };
  // calibration: channel maxima of rows [r0, r0 + rows) of a bf16 tensor into the smoothing slot `slot`
  auto cal = [&](const bf16_t* x, int ld, int r0, int rows, int K, int64_t slot) {
    return td_col_amax_launch(x + (size_t)r0 * ld, ld, rows, K, wroot->sm_ax + slot, s);
  };
  for (int i = 0; i < L; ++i) {
    const DoubleW& w = f->dbl[i];
    const bf16_t* mi = mod + (size_t)i * 12 * D;  // img: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    const bf16_t* mc = mi + 6 * D;                // ctx: same order
    np.shiftA = mc; np.scaleA = mc + D; np.shiftB = mi; np.scaleB = mi + D;
    const int64_t sd = sm_dbl(root, i);      // this block's smoothing slots: qkv_img, qkv_ctx, ff1_img, ff1_ctx [D each], ff2_img, ff2_ctx [M each]
    const int* sx = root->sm_ext + (size_t)4 * i * SM_EXT;      // ... and their replicated-channel tables, same order
    norm_for(m8 & TD_FP8_QKV, root->sm_inv16 + sd + D, root->sm_inv16 + sd, sx + SM_EXT, sx);
    TD_TRY(norm_rows(f, s, np));
    if (calib) { TD_TRY(cal(f->xn, D, 0, T, D, sd + D)); TD_TRY(cal(f->xn, D, T, Si, D, sd)); }
    bf16_t* xn_img = f->xn + (size_t)T * D;
    if (m8 & TD_FP8_QKV) {
      const DoubleW8& w8 = root->dbl8[i];
      TD_TRY(gemm2_8(f, s, f->xq + (size_t)T * DX, f->xs + T, w8.qkv_img, w.qkv_img_b, f->qkv + (size_t)T * 3 * D, Si,
                     f->xq, f->xs, w8.qkv_ctx, w.qkv_ctx_b, f->qkv, T, DX, 3 * D, 3 * D, DX));
    } else {
      TD_TRY(gemm2(f, s, xn_img, w.qkv_img_w, w.qkv_img_b, f->qkv + (size_t)T * 3 * D, Si,
                   f->xn, w.qkv_ctx_w, w.qkv_ctx_b, f->qkv, T, D, 3 * D, 3 * D, D));
    }
    rp.wqA = w.norm_added_q; rp.wkA = w.norm_added_k; rp.wqB = w.norm_q; rp.wkB = w.norm_k;
    if (!rope_in_pack) TD_TRY(qk_rope(f, s, rp));
    ap.score_bound = use_bound && (size_t)i < root->dbl_bound.size() ? root->dbl_bound[i] : 0.f;
    ap.O = f->attn; ap.ldo = D;
    // history scales: the attention epilogue writes its output as int8 under the previous step's per-token scale (the out-proj's A operand)
    const bool ao_hist = use_hist && (m8 & TD_FP8_OUT);
    float* asc_o = f->hs_scale + (size_t)(L + Ls + i) * f->hs_cap;
    unsigned* aam_o = f->hs_amax + (size_t)(L + Ls + i) * f->hs_cap;
    if (ao_hist) { ap.q8 = f->aq; ap.ldq8 = D; ap.q8_inv = f->hs_inv + (size_t)(L + Ls + i) * f->hs_cap; ap.q8_amax = aam_o; }
    TD_TRY(attn(f, s, ap, rope_in_pack ? &rp : nullptr, href_in ? href_in + (size_t)i * href_blk : nullptr, href_out ? href_out + (size_t)i * href_blk : nullptr));
    ap.q8 = nullptr;
    if (m8 & TD_FP8_OUT) {
      const DoubleW8& w8 = root->dbl8[i];
      if (!ao_hist) TD_TRY(quant_act(f, s, f->attn, D, S, D, hist_mode ? aam_o : nullptr));
      const float* asc = ao_hist ? asc_o : f->as_;
      TD_TRY(gemm2_8(f, s, f->aq + (size_t)T * D, asc + T, w8.out_img, w.out_img_b, h_img, Si,
                     f->aq, asc, w8.out_ctx, w.out_ctx_b, h, T, D, D, D, D, TD_ACT_NONE, mi + 2 * D, mc + 2 * D, true));
    } else {
      TD_TRY(gemm2(f, s, f->attn + (size_t)T * D, w.out_img_w, w.out_img_b, h_img, Si,
                   f->attn, w.out_ctx_w, w.out_ctx_b, h, T, D, D, D, D, TD_ACT_NONE, mi + 2 * D, mc + 2 * D, true));
    }
    np.shiftA = mc + 3 * D; np.scaleA = mc + 4 * D; np.shiftB = mi + 3 * D; np.scaleB = mi + 4 * D;
    norm_for(m8 & TD_FP8_FF1, root->sm_inv16 + sd + 3 * D, root->sm_inv16 + sd + 2 * D, sx + 3 * SM_EXT, sx + 2 * SM_EXT);
    TD_TRY(norm_rows(f, s, np));
    if (calib) { TD_TRY(cal(f->xn, D, 0, T, D, sd + 3 * D)); TD_TRY(cal(f->xn, D, T, Si, D, sd + 2 * D)); }
    const bool ff_hist = use_hist && (m8 & TD_FP8_FF1) && (m8 & TD_FP8_FF2);
    float* hsc = f->hs_scale + (size_t)i * f->hs_cap;
    float* hiv = f->hs_inv + (size_t)i * f->hs_cap;
    unsigned* ham = f->hs_amax + (size_t)i * f->hs_cap;
    if (m8 & TD_FP8_FF1) {
      const DoubleW8& w8 = root->dbl8[i];
      Q8Out q_img, q_ctx;
      q_img.q = f->aq + (size_t)T * M; q_img.ld = M; q_img.inv = hiv + T; q_img.amax = ham + T;
      q_ctx.q = f->aq; q_ctx.ld = M; q_ctx.inv = hiv; q_ctx.amax = ham;
      if (sm_on) { q_img.smooth = root->sm_inv16 + sd + 4 * D; q_ctx.smooth = root->sm_inv16 + sd + 4 * D + M; }
      TD_TRY(gemm2_8(f, s, f->xq + (size_t)T * DX, f->xs + T, w8.ff1_img, w.ff1_img_b, f->mlp + (size_t)T * M, Si,
                     f->xq, f->xs, w8.ff1_ctx, w.ff1_ctx_b, f->mlp, T, DX, M, M, DX, TD_ACT_GELU_TANH, nullptr, nullptr, false,
                     ff_hist ? &q_img : nullptr, ff_hist ? &q_ctx : nullptr));
    } else {
      TD_TRY(gemm2(f, s, xn_img, w.ff1_img_w, w.ff1_img_b, f->mlp + (size_t)T * M, Si,
                   f->xn, w.ff1_ctx_w, w.ff1_ctx_b, f->mlp, T, D, M, M, D, TD_ACT_GELU_TANH));
      if (calib) { TD_TRY(cal(f->mlp, M, 0, T, M, sd + 4 * D + M)); TD_TRY(cal(f->mlp, M, T, Si, M, sd + 4 * D)); }
    }
    if (m8 & TD_FP8_FF2) {
      const DoubleW8& w8 = root->dbl8[i];
      if (!ff_hist) {
        if (sm_on) {      // the two streams meet different weights: their own factors
          TD_TRY(quant_act(f, s, f->mlp, M, T, M, hist_mode ? ham : nullptr, root->sm_inv + sd + 4 * D + M, 0));
          TD_TRY(quant_act(f, s, f->mlp, M, Si, M, hist_mode ? ham : nullptr, root->sm_inv + sd + 4 * D, T));
        } else {
          TD_TRY(quant_act(f, s, f->mlp, M, S, M, hist_mode ? ham : nullptr));
        }
      }
      const float* asc = ff_hist ? hsc : f->as_;
      TD_TRY(gemm2_8(f, s, f->aq + (size_t)T * M, asc + T, w8.ff2_img, w.ff2_img_b, h_img, Si,
                     f->aq, asc, w8.ff2_ctx, w.ff2_ctx_b, h, T, M, D, D, M, TD_ACT_NONE, mi + 5 * D, mc + 5 * D, true));
    } else {
      TD_TRY(gemm2(f, s, f->mlp + (size_t)T * M, w.ff2_img_w, w.ff2_img_b, h_img, Si,
                   f->mlp, w.ff2_ctx_w, w.ff2_ctx_b, h, T, M, D, D, M, TD_ACT_NONE, mi + 5 * D, mc + 5 * D, true));
    }
  }

  const bool fused_split = (3 * D) % 256 == 0;
  for (int i = 0; i < Ls; ++i) {
    const SingleW& w = f->sgl[i];
    const bf16_t* ms = mod + (size_t)L * 12 * D + (size_t)i * 3 * D;  // shift, scale, gate
    np.shiftA = np.shiftB = ms; np.scaleA = np.scaleB = ms + D;
    const int64_t ss = sm_sgl(root, i);      // this block's smoothing slots: w1 [D], w2 [D + M] (its first D channels -- the attention half -- stay 1)
    const int* sxs = root->sm_ext + (size_t)(4 * L + i) * SM_EXT;
    norm_for(m8 & TD_FP8_SINGLE_IN, root->sm_inv16 + ss, root->sm_inv16 + ss, sxs, sxs);
    TD_TRY(norm_rows(f, s, np));
    if (calib) TD_TRY(cal(f->xn, D, 0, S, D, ss));
    const bool sg_hist = use_hist && fused_split && (m8 & TD_FP8_SINGLE_IN) && (m8 & TD_FP8_SINGLE_OUT);
    float* hsc = f->hs_scale + (size_t)(L + i) * f->hs_cap;
    float* hiv = f->hs_inv + (size_t)(L + i) * f->hs_cap;
    unsigned* ham = f->hs_amax + (size_t)(L + i) * f->hs_cap;
    if (m8 & TD_FP8_SINGLE_IN) {
      const SingleW8& w8 = root->sgl8[i];
      if (fused_split) {
        Q8Out q_mlp;
        q_mlp.q = f->aq + D; q_mlp.ld = D + M; q_mlp.inv = hiv; q_mlp.amax = ham;      // the mlp half of [attn | mlp], int8, straight from the epilogue
        if (sm_on) q_mlp.smooth = root->sm_inv16 + ss + 2 * D - 3 * D;      // indexed by the launch's absolute output column n >= 3 D: w2's MLP channels start at ss + D + D
        TD_TRY(gemm8(f, s, f->xq, DX, f->xs, w8.w1, w.b1, f->qkv, 3 * D, S, 3 * D + M, DX, TD_ACT_NONE, nullptr, nullptr, 0,
                     f->cat + D, D + M, TD_ACT_GELU_TANH, 3 * D, sg_hist ? &q_mlp : nullptr));
      } else {
        Fp8Mat wa = w8.w1, wb = w8.w1;
        wb.q += (size_t)3 * D * DX; wb.s += 3 * D;
        TD_TRY(gemm8(f, s, f->xq, DX, f->xs, wa, w.b1, f->qkv, 3 * D, S, 3 * D, DX));
        TD_TRY(gemm8(f, s, f->xq, DX, f->xs, wb, w.b1 + 3 * D, f->cat + D, D + M, S, M, DX, TD_ACT_GELU_TANH));
      }
    } else if (fused_split) {
      TdGemmParams gp;
      gp.A = f->xn; gp.lda = D; gp.W = w.w1; gp.bias = w.b1; gp.M = S; gp.N = 3 * D + M; gp.K = D;
      gp.C = f->qkv; gp.ldc = 3 * D; gp.act = TD_ACT_NONE;
      gp.C2 = f->cat + D; gp.ldc2 = D + M; gp.act2 = TD_ACT_GELU_TANH; gp.n_split = 3 * D;
      TD_TRY(gemm_p(f, s, gp));
      if (calib) TD_TRY(cal(f->cat + D, D + M, 0, S, M, ss + 2 * D));
    } else {
      TD_TRY(gemm(f, s, f->xn, D, w.w1, w.b1, f->qkv, 3 * D, S, 3 * D, D));
      TD_TRY(gemm(f, s, f->xn, D, w.w1 + (size_t)3 * D * D, w.b1 + 3 * D, f->cat + D, D + M, S, M, D, TD_ACT_GELU_TANH));
    }
    rp.wqA = rp.wqB = w.norm_q; rp.wkA = rp.wkB = w.norm_k;
    if (!rope_in_pack) TD_TRY(qk_rope(f, s, rp));
    ap.score_bound = use_bound && (size_t)i < root->sgl_bound.size() ? root->sgl_bound[i] : 0.f;
    ap.O = f->cat; ap.ldo = D + M;
    if (sg_hist) { ap.q8 = f->aq; ap.ldq8 = D + M; ap.q8_inv = hiv; ap.q8_amax = ham; }   // the attention half of [attn | mlp] as int8, same per-token scale
    TD_TRY(attn(f, s, ap, rope_in_pack ? &rp : nullptr, href_in ? href_in + (size_t)(L + i) * href_blk : nullptr, href_out ? href_out + (size_t)(L + i) * href_blk : nullptr));
    ap.q8 = nullptr;
    if (m8 & TD_FP8_SINGLE_OUT) {
      if (sg_hist) {
        // both halves of the operand are in f->aq already: the mlp half from the W1 epilogue, the attention half from the attention epilogue
      } else {
        TD_TRY(quant_act(f, s, f->cat, D + M, S, D + M, hist_mode ? ham : nullptr, sm_on ? root->sm_inv + ss + D : nullptr));
      }
      TD_TRY(gemm8(f, s, f->aq, D + M, sg_hist ? hsc : f->as_, root->sgl8[i].w2, w.b2, h, D, S, D, D + M, TD_ACT_NONE, ms + 2 * D, h, D));
    } else {
      TD_TRY(gemm(f, s, f->cat, D + M, w.w2, w.b2, h, D, S, D, D + M, TD_ACT_NONE, ms + 2 * D, h, D));
    }
  }

  // AdaLayerNormContinuous: chunk order (scale, shift); the latents' image rows only (reference tokens have no velocity)
  const bf16_t* mf = mod + (size_t)L * 12 * D + (size_t)Ls * 3 * D;
  TdNormParams nf = np;
  nf.q = nullptr;   // the final projection stays bf16
  nf.smoothA = nf.smoothB = nullptr; nf.extA = nf.extB = nullptr; nf.ext_n = 0;
  nf.x = h_img; nf.y = f->xn; nf.rows = So; nf.split = 0;
  nf.scaleA = nf.scaleB = mf; nf.shiftA = nf.shiftB = mf + D;
  TD_TRY(norm_rows(f, s, nf));
  TD_TRY(gemm(f, s, f->xn, D, f->proj_w, f->proj_b, (bf16_t*)velocity, C, So, C, D));
  if (calib) TD_TRY(finish_smoothing(wroot, s));      // (synchronises s; bumps the history epoch)
  if (hist_mode) { f->hs_step = step; f->hs_T = T; f->hs_S = S; f->hs_epoch = root->hist_epoch; } else f->hs_step = -1;
  if (href_on) { f->href_cur ^= 1; f->href_step = step; f->href_T = T; f->href_S = S; f->href_epoch = root->hist_epoch; } else f->href_step = -1;
  return TD_OK;
}

// Per-launch HIP-event trace.  begin: arm (events are created once); end: synchronise the stream and
// return, per category, launch count / summed milliseconds / summed algorithmic FLOPs.
int td_flux_trace_begin(td_flux* f, int max_launches) {
  TD_CHECK_ARG(f && max_launches > 0, "td_flux_trace_begin: bad arguments");
  while ((int)f->ev_pool.size() < 2 * max_launches) {
    hipEvent_t ev;
    TD_CHECK_HIP(hipEventCreate(&ev));
    f->ev_pool.push_back(ev);
  }
  f->trace.clear();
  f->trace.reserve(max_launches);
  f->tracing = true;
  return TD_OK;
}

int td_flux_trace_end(td_flux* f, void* stream, int64_t* counts, double* ms, double* flops) {
  TD_CHECK_ARG(f && counts && ms && flops, "td_flux_trace_end: null argument");
  f->tracing = false;
  TD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (int c = 0; c < TD_TRACE_NCAT; ++c) { counts[c] = 0; ms[c] = 0.0; flops[c] = 0.0; }
  for (size_t i = 0; i < f->trace.size(); ++i) {
    float t = 0.f;
    TD_CHECK_HIP(hipEventElapsedTime(&t, f->ev_pool[2 * i], f->ev_pool[2 * i + 1]));
    const int c = f->trace[i].cat;
    counts[c] += 1; ms[c] += t; flops[c] += f->trace[i].flops;
  }
  return TD_OK;
}

}  // extern "C"

namespace {

// The blend operands of one image in FluxInpaintPipeline's loop (td_flux_denoise_inpaint); a null InpaintBlend is the plain Euler step.
struct InpaintBlend {
  const void* z;       // packed clean image latents
  const void* noise;   // packed start noise
  const void* mask;    // packed 0 / 1 mask (td_flux_inpaint_mask)
};

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// blend k's buffers: present, 16-byte aligned, and clear of every latents buffer the loop writes
int check_blend(const char* fn, td_flux* const* fs, void* const* latents, int count, int k, const InpaintBlend& b) {
  TD_CHECK_ARG(b.z && b.noise && b.mask, "%s: image %d: image_latents, noise and mask are required", fn, k);
  const size_t bytes = (size_t)fs[k]->S_img * fs[k]->Cout * sizeof(bf16_t);
  const void* bufs[3] = {b.z, b.noise, b.mask};
  static const char* names[3] = {"image_latents", "noise", "mask"};
  for (int j = 0; j < 3; ++j) {
    TD_CHECK_ARG((uintptr_t)bufs[j] % 16 == 0, "%s: image %d: %s must be 16-byte aligned", fn, k, names[j]);
    for (int l = 0; l < count; ++l)
      TD_CHECK_ARG(!overlaps(bufs[j], bytes, latents[l], (size_t)fs[l]->S_img * fs[l]->Cout * sizeof(bf16_t)),
                   "%s: image %d: %s overlaps the latents of image %d (the loop writes them in place)", fn, k, names[j], l);
  }
  return TD_OK;
}

// the scheduler step of loop step i (of n) after the forward wrote f->vout: Euler, or Euler + scale_noise + mask blend
int scheduler_step(td_flux* f, void* latents, const float* sigmas, int i, int n, const InpaintBlend* b, void* stream) {
  const long long count = (long long)f->S_img * f->Cout;
  if (!b) return td_euler_step_launch((bf16_t*)latents, f->vout, sigmas[i + 1] - sigmas[i], count, (hipStream_t)stream);
  return td_flux_inpaint_step_launch((bf16_t*)latents, f->vout, (const bf16_t*)b->z, i < n - 1 ? (const bf16_t*)b->noise : nullptr,
                                     (const bf16_t*)b->mask, sigmas[i + 1] - sigmas[i], sigmas[i + 1], count, (hipStream_t)stream);
}

// The FluxPipeline.__call__ loop: for i: v = transformer(x, t_i); x = bf16(float(x) + (sigma_{i+1}-sigma_i) float(v)).
// latents [S_img, out_channels] bf16, updated in place; sigmas: n+1 host floats.  blend: FluxInpaintPipeline's step instead.
int denoise_loop(td_flux* f, void* latents, const float* sigmas, int n, const InpaintBlend* blend, void* stream) {
  for (int i = 0; i < n; ++i) {
    TD_TRY(td_flux_forward(f, latents, i, f->vout, stream));
    TD_TRY(scheduler_step(f, latents, sigmas, i, n, blend, stream));
  }
  return TD_OK;
}

// Several independent images in flight: contexts fs[k] (a parent and its forks) advance step by step, each on its own
// stream, so the tail of one image's kernels (grids of 1.6 - 3.2 rounds of the 256 CUs) is filled by the other's.
// blends: NULL, or one InpaintBlend per context.
int denoise_multi_loop(td_flux* const* fs, void* const* latents, int count, const float* sigmas, int n, const InpaintBlend* blends,
                       void* const* streams) {
  // With several images in flight the attention of each runs as a plain grid (one workgroup per item): its second, 59 %-empty
  // round is exactly what the other images' kernels fill, while the persistent form holds every CU for its whole duration
  // and shuts them out (measured, 3 in flight: 0.698 images/s persistent vs 0.71 plain; one image alone: 0.678 vs 0.655).
  static const char* force = getenv("TD_FLUX_INFLIGHT_ATTN");      // experiments only: 0 / 1 forces the attention form used with images in flight
  const int multi_variant = force ? atoi(force) : 1;
  for (int k = 0; k < count; ++k) { fs[k]->attn_variant = count > 1 ? multi_variant : 0; fs[k]->shared_chip = count > 1; }
  int rc = TD_OK;
  for (int i = 0; i < n && rc == TD_OK; ++i)
    for (int k = 0; k < count && rc == TD_OK; ++k) {
      td_flux* f = fs[k];
      rc = td_flux_forward(f, latents[k], i, f->vout, streams[k]);
      if (rc == TD_OK) rc = scheduler_step(f, latents[k], sigmas, i, n, blends ? &blends[k] : nullptr, streams[k]);
    }
  for (int k = 0; k < count; ++k) { fs[k]->attn_variant = 0; fs[k]->shared_chip = false; }
  return rc;
}

}  // namespace

extern "C" {

int td_flux_denoise(td_flux* f, void* latents, const float* sigmas, int n, void* stream) {
  TD_CHECK_ARG(f && latents && sigmas, "td_flux_denoise: null argument");
  TD_CHECK_ARG(n > 0 && n <= f->n_steps, "td_flux_denoise: n=%d exceeds the %d prepared timesteps", n, f->n_steps);
  return denoise_loop(f, latents, sigmas, n, nullptr, stream);
}

// FluxKontextPipeline's loop with true classifier-free guidance: per step the transformer under the positive and under the negative
// conditioning (two contexts, ONE stream), then td_flux_cfg_step_bf16.
int td_flux_denoise_cfg(td_flux* pos, td_flux* neg, void* latents, const float* sigmas, int n, float scale, void* stream) {
  TD_CHECK_ARG(pos && neg && latents && sigmas, "td_flux_denoise_cfg: null argument");
  TD_CHECK_ARG(pos != neg, "td_flux_denoise_cfg: the positive and the negative context are the same object (fork one from the other)");
  TD_CHECK_ARG(pos->cond_set && neg->cond_set, "td_flux_denoise_cfg: both contexts need td_flux_set_condition");
  TD_CHECK_ARG(pos->S_img == neg->S_img && pos->Cout == neg->Cout, "td_flux_denoise_cfg: the contexts disagree on the latents: S_img %d / %d, out_channels %d / %d",
               pos->S_img, neg->S_img, pos->Cout, neg->Cout);
  TD_CHECK_ARG(pos->S_ref == neg->S_ref, "td_flux_denoise_cfg: the contexts hold %d / %d reference tokens (set the image's reference tokens on both, or on neither)",
               pos->S_ref, neg->S_ref);
  TD_CHECK_ARG(pos->n_steps == neg->n_steps, "td_flux_denoise_cfg: the contexts are prepared for %d / %d timesteps", pos->n_steps, neg->n_steps);
  TD_CHECK_ARG(n > 0 && n <= pos->n_steps, "td_flux_denoise_cfg: n=%d exceeds the %d prepared timesteps", n, pos->n_steps);
  const long long count = (long long)pos->S_img * pos->Cout;
  TD_CHECK_ARG(!overlaps(latents, (size_t)count * 2, pos->vout, (size_t)count * 2) && !overlaps(latents, (size_t)count * 2, neg->vout, (size_t)count * 2),
               "td_flux_denoise_cfg: latents overlap a context's velocity buffer");
  for (int i = 0; i < n; ++i) {
    TD_TRY(td_flux_forward(pos, latents, i, pos->vout, stream));
    TD_TRY(td_flux_forward(neg, latents, i, neg->vout, stream));
    TD_TRY(td_flux_cfg_step_launch((bf16_t*)latents, pos->vout, neg->vout, scale, sigmas[i + 1] - sigmas[i], count, (hipStream_t)stream));
  }
  return TD_OK;
}

int td_flux_denoise_inpaint(td_flux* f, void* latents, const float* sigmas, int n, const void* image_latents, const void* noise,
                            const void* mask, void* stream) {
  TD_CHECK_ARG(f && latents && sigmas, "td_flux_denoise_inpaint: null argument");
  TD_CHECK_ARG(n > 0 && n <= f->n_steps, "td_flux_denoise_inpaint: n=%d exceeds the %d prepared timesteps", n, f->n_steps);
  const InpaintBlend b{image_latents, noise, mask};
  void* const lat[1] = {latents};
  TD_TRY(check_blend("td_flux_denoise_inpaint", &f, lat, 1, 0, b));
  return denoise_loop(f, latents, sigmas, n, &b, stream);
}

int td_flux_denoise_multi(td_flux* const* fs, void* const* latents, int count, const float* sigmas, int n, void* const* streams) {
  TD_CHECK_ARG(fs && latents && sigmas && streams && count > 0, "td_flux_denoise_multi: null argument");
  for (int k = 0; k < count; ++k)
    TD_CHECK_ARG(fs[k] && latents[k] && n > 0 && n <= fs[k]->n_steps, "td_flux_denoise_multi: context %d is not prepared for %d steps", k, n);
  return denoise_multi_loop(fs, latents, count, sigmas, n, nullptr, streams);
}

int td_flux_denoise_multi_inpaint(td_flux* const* fs, void* const* latents, int count, const float* sigmas, int n,
                                  const void* const* image_latents, const void* const* noise, const void* const* mask, void* const* streams) {
  TD_CHECK_ARG(fs && latents && sigmas && streams && image_latents && noise && mask && count > 0, "td_flux_denoise_multi_inpaint: null argument");
  for (int k = 0; k < count; ++k)
    TD_CHECK_ARG(fs[k] && latents[k] && n > 0 && n <= fs[k]->n_steps, "td_flux_denoise_multi_inpaint: context %d is not prepared for %d steps", k, n);
  std::vector<InpaintBlend> blends(count);
  for (int k = 0; k < count; ++k) {
    blends[k] = InpaintBlend{image_latents[k], noise[k], mask[k]};
    TD_TRY(check_blend("td_flux_denoise_multi_inpaint", fs, latents, count, k, blends[k]));
  }
  return denoise_multi_loop(fs, latents, count, sigmas, n, blends.data(), streams);
}

}  // extern "C"
