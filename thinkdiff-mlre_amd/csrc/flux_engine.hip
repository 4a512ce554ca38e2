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
//
// Files: csrc/flux_model.h holds the two structures -- FluxModel (weights, numeric configuration, LoRA registry; shared) and td_flux (one
// image's context: workspace, conditioning, schedule, history, trace).  csrc/flux_model.hip holds everything that touches only the model;
// this file holds everything that runs on a context: create / fork / destroy, conditioning, schedule, the forward, the denoise loops, the trace.
// A ControlNet side network (td_flux_controlnet_*) is a second KIND of model run by the same block loop (run_blocks): its contexts keep block
// samples, and a main context with one attached adds them behind its own blocks (td_flux_attach_controlnet, td_flux_residual_inject_bf16); with up
// to TD_MAX_CONTROLNETS attached it adds their bf16 sum, one launch per block (td_flux_attach_controlnets, td_flux_residual_inject_multi_bf16).
// IP-Adapter slots (td_flux_ip_adapter_*: the model's; td_flux_set_ip_image_embeds: a context's image prompt -> tokens and every double block's
// K / V, once per image) add, inside a double block, td_ip_attention of the image rows' un-rotated query and one add behind the FF.
// The first-block cache (td_flux_set_block_cache*; kernels in csrc/block_cache.hip) decides behind double block 0 whether the forward runs its
// remaining blocks or adds the tail the last computed forward left -- the one place the forward waits for the device.
#include <cmath>
#include <cstring>
#include <functional>

#include "flux_model.h"

namespace {

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
// The same hint picks the tile by CU time (td_gemm_plan).  The tile is decided HERE, once, and handed to the launcher, so the trace category is the
// kernel that runs; up to 64 rows the launcher still decides between its weight-stream and tile kernels itself (it does so only without an override).
int gemm_p(td_flux* f, hipStream_t s, TdGemmParams p) {
  p.no_tail = f->shared_chip;
  const int rows = p.M + p.g_M;
  const int cfg = p.cfg >= 0 ? p.cfg : td_gemm_plan(rows, p.N, (p.fp8 || p.i8) ? p.K / 2 : p.K,      // (8-bit operands: tiles are chosen by bytes)
                                                    p.no_tail, p.i8 ? TD_OPERAND_INT8 : p.fp8 ? TD_OPERAND_E4M3 : TD_OPERAND_BF16);
  if (rows > 64) p.cfg = cfg;
  TraceScope ts(f, s, cfg == 0 ? TD_TRACE_GEMM_MAIN : cfg == 3 ? TD_TRACE_GEMM_288 : TD_TRACE_GEMM_OTHER, 2.0 * rows * p.N * p.K);
  return td_gemm_launch(p, s);
}

// The input rows of a Linear in the forms the engine holds them in: bf16 (x), and / or 8-bit rows with one scale per row (q, qs).  Which form a
// Linear reads is the helper's decision, not the call site's.
struct Rows {
  const bf16_t* x = nullptr; int ldx = 0;
  const uint8_t* q = nullptr; int ldq = 0; const float* qs = nullptr;
  Rows from(int r) const {
    Rows a = *this;
    if (x) a.x += (size_t)r * ldx;
    if (q) { a.q += (size_t)r * ldq; a.qs += r; }
    return a;
  }
};
Rows bf16_rows(const void* x, int ld) { Rows a; a.x = (const bf16_t*)x; a.ldx = ld; return a; }

// int8 copy of the activated result under scales fixed in advance (TdGemmParams::q8), beside the bf16 output.  A pair launch takes the text rows
// first, as every joint buffer does; `smooth` / `smooth_ctx`: the next Linear's smoothing factors of the image / the text stream.
struct Q8Out { uint8_t* q = nullptr; int ld = 0; const float* inv = nullptr; unsigned* amax = nullptr; const bf16_t *smooth = nullptr, *smooth_ctx = nullptr; };

// Where a Linear's result goes and what happens to it on the way: y = act(x W^T + b) [* gate] [+ c].
struct Epilogue {
  bf16_t* c = nullptr; int ldc = 0;
  int act = TD_ACT_NONE;
  const bf16_t *gate = nullptr, *gate_ctx = nullptr;      // per output channel; a pair launch: of the image / of the text stream
  bool residual = false;                                  // y += c (in place)
  const bf16_t* res = nullptr; int ldr = 0;               // y += res (another buffer; same rounding points: the Linear's output rounds, then the sum)
  bf16_t* c2 = nullptr; int ldc2 = 0, act2 = TD_ACT_NONE, n_split = 0;      // output columns >= n_split go to c2 under act2
  const Q8Out* q8 = nullptr;                              // 8-bit form only
  static Epilogue to(bf16_t* c, int ldc, int act = TD_ACT_NONE) { Epilogue o; o.c = c; o.ldc = ldc; o.act = act; return o; }
  Epilogue& gated_residual(const bf16_t* g, const bf16_t* g_ctx = nullptr) { gate = g; gate_ctx = g_ctx; residual = true; return *this; }
  Epilogue& plus(const bf16_t* r, int ld) { res = r; ldr = ld; return *this; }
  Epilogue& split(int n, bf16_t* c2_, int ldc2_, int act2_) { n_split = n; c2 = c2_; ldc2 = ldc2_; act2 = act2_; return *this; }
  Epilogue& int8_out(const Q8Out* q) { q8 = q; return *this; }
};

// One Linear over `rows` rows of `a`: on 8-bit operands when the model's precision, Linear-class mask and calibration state say so, else in bf16.
int linear(td_flux* f, hipStream_t s, const FluxLinear& l, const Rows& a, int rows, const Epilogue& o) {
  const FluxModel* m = f->m;
  TdGemmParams p;
  p.M = rows; p.N = l.N; p.bias = l.b;
  p.C = o.c; p.ldc = o.ldc; p.act = o.act; p.gate = o.gate;
  if (o.residual) { p.res = o.c; p.ldr = o.ldc; }
  else if (o.res) { p.res = o.res; p.ldr = o.ldr; }
  p.C2 = o.c2; p.ldc2 = o.ldc2; p.act2 = o.act2; p.n_split = o.n_split;
  if (flux_mask8(m) & l.cls) {
    p.fp8 = m->precision == TD_PRECISION_FP8_E4M3; p.i8 = m->precision == TD_PRECISION_INT8;
    p.A = (const bf16_t*)a.q; p.lda = a.ldq; p.a_scale = a.qs;
    p.W = (const bf16_t*)l.w8.q; p.w_scale = l.w8.s; p.K = flux_k8(m, l);
    if (o.q8) { p.q8 = o.q8->q; p.ldq8 = o.q8->ld; p.q8_inv = o.q8->inv; p.q8_amax = o.q8->amax; p.q8_smooth = o.q8->smooth; }
  } else {
    p.A = a.x; p.lda = a.ldx; p.W = l.w; p.K = l.K;
  }
  return gemm_p(f, s, p);
}

// The image-stream and the text-stream Linear of a double block in one launch (problem 0 = image rows).  `a` and the outputs are joint buffers:
// T text rows, then Si image rows.
int linear2(td_flux* f, hipStream_t s, const FluxLinear& img, const FluxLinear& ctx, const Rows& a, int T, int Si, const Epilogue& o) {
  const FluxModel* m = f->m;
  const Rows ai = a.from(T);
  TdGemmParams p;
  p.M = Si; p.g_M = T; p.N = img.N; p.act = o.act;
  p.bias = img.b; p.g_bias = ctx.b;
  p.C = o.c + (size_t)T * o.ldc; p.g_C = o.c; p.ldc = p.ldr = o.ldc;
  p.gate = o.gate; p.g_gate = o.gate_ctx;
  if (o.residual) { p.res = p.C; p.g_res = p.g_C; }
  if (flux_mask8(m) & img.cls) {
    p.fp8 = m->precision == TD_PRECISION_FP8_E4M3; p.i8 = m->precision == TD_PRECISION_INT8;
    p.A = (const bf16_t*)ai.q; p.a_scale = ai.qs; p.g_A = (const bf16_t*)a.q; p.g_a_scale = a.qs; p.lda = a.ldq;
    p.W = (const bf16_t*)img.w8.q; p.w_scale = img.w8.s; p.g_W = (const bf16_t*)ctx.w8.q; p.g_w_scale = ctx.w8.s; p.K = flux_k8(m, img);
    if (o.q8) {
      const Q8Out& q = *o.q8;
      p.q8 = q.q + (size_t)T * q.ld; p.ldq8 = q.ld; p.q8_inv = q.inv + T; p.q8_amax = q.amax + T; p.q8_smooth = q.smooth;
      p.g_q8 = q.q; p.g_q8_inv = q.inv; p.g_q8_amax = q.amax; p.g_q8_smooth = q.smooth_ctx;
    }
  } else {
    p.A = ai.x; p.g_A = a.x; p.lda = a.ldx; p.W = img.w; p.g_W = ctx.w; p.K = img.K;
  }
  return gemm_p(f, s, p);
}

// N may exceed the 4 GiB buffer-descriptor range of W (the fused modulation matrix is 6.5 GB):
// walk it in column chunks.
int linear_big_n(td_flux* f, hipStream_t s, const FluxLinear& l, const Rows& a, int rows, bf16_t* C, int ldc) {
  const int chunk = 131072;
  for (int n0 = 0; n0 < l.N; n0 += chunk) {
    FluxLinear part = l;
    part.w += (int64_t)n0 * l.K; part.b += n0; part.N = l.N - n0 < chunk ? l.N - n0 : chunk;
    TD_TRY(linear(f, s, part, a, rows, Epilogue::to(C + n0, ldc)));
  }
  return 0;
}

struct Span { int r0, rows; };      // rows [r0, r0 + rows) of a joint buffer

// per-token quantisation of rows `sp` of a bf16 activation matrix [*, K] into the same rows of f->aq / f->as_; col_mul: int8 smoothing factors (1 / s)
int quant_act(td_flux* f, hipStream_t s, const bf16_t* x, int K, Span sp, unsigned* amax_out = nullptr, const float* col_mul = nullptr) {
  TraceScope ts(f, s, TD_TRACE_NORM, 0.0);
  return td_quant_rows_fp8_launch(x + (size_t)sp.r0 * K, K, f->aq + (size_t)sp.r0 * K, K, f->as_ + sp.r0, sp.rows, K, s,
                                  f->m->precision == TD_PRECISION_INT8, amax_out ? amax_out + sp.r0 : nullptr, col_mul);
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
  if (f->m->attn_mode == TD_ATTENTION_FP8) {      // both products on the e4m3 MFMA: pack pass + persistent kernel (csrc/attention_fp8.hip)
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

// A/B switches of the forward (experiments, and the bit-identity tests).  Tests and tools/ab_policy.py flip them inside one process, so all
// are read per call; a few getenv per forward are noise next to ~600 launches.
struct Switches {
  int attn_tune;             // TD_ATTN_TUNE: variant bits of the attention kernel (0x400: the score-bound form on its 32x32x16 body)
  bool attn8_no_fuse;        // TD_ATTN8_NO_FUSE: the 8-bit attention takes q / k from td_qk_norm_rope instead of its own pack pass
  bool attn8_no_href;        // TD_ATTN8_NO_HREF: no history reference points
  bool attn_no_bound;        // TD_ATTN_NO_BOUND: the running-maximum form of the bf16 attention
  static Switches read() {
    const char* const at = getenv("TD_ATTN_TUNE");
    const int tune = at ? (int)strtol(at, nullptr, 0) & ~0xff : 0;
    return {tune, getenv("TD_ATTN8_NO_FUSE") != nullptr, getenv("TD_ATTN8_NO_HREF") != nullptr, getenv("TD_ATTN_NO_BOUND") != nullptr};
  }
};

// a context's activation workspace (one allocation)
int alloc_workspace(td_flux* f) {
  const FluxModel* m = f->m;
  const TdFluxConfig* cfg = &m->cfg;
  const int64_t D = m->D, M = m->M;
  const int max_img_tokens = m->max_img, max_txt_tokens = m->max_txt + (m->num_mode > 0 ? 1 : 0);      // (a union ControlNet prepends its mode row)
  const int64_t S = (int64_t)max_img_tokens + max_txt_tokens;
  const int64_t n = m->max_steps;
  struct Req { void** p; int64_t bytes; };
  std::vector<Req> reqs = {
      {(void**)&f->h, S * D * 2}, {(void**)&f->xn, S * D * 2}, {(void**)&f->qkv, S * 3 * D * 2},
      {(void**)&f->attn, S * D * 2}, {(void**)&f->mlp, S * M * 2}, {(void**)&f->cat, S * (D + M) * 2},
      {(void**)&f->ctx, (int64_t)max_txt_tokens * D * 2}, {(void**)&f->vout, (int64_t)max_img_tokens * m->Cout * 2},
      {(void**)&f->xin, m->Ccond > 0 ? (int64_t)max_img_tokens * m->Cin * 2 : 0},
      {(void**)&f->xref, m->Ccond == 0 ? (int64_t)max_img_tokens * m->Cout * 2 : 0},
      {(void**)&f->cn_E, m->controlnet ? (int64_t)max_img_tokens * D * 2 : 0},
      {(void**)&f->cn_samples, m->controlnet ? (int64_t)(cfg->num_layers + cfg->num_single_layers) * max_img_tokens * D * 2 : 0},
      {(void**)&f->tproj, n * 256 * 2}, {(void**)&f->tmid, n * D * 2}, {(void**)&f->te, n * D * 2},
      {(void**)&f->gproj, 256 * 2}, {(void**)&f->gmid, (int64_t)D * 2}, {(void**)&f->ge, (int64_t)D * 2},
      {(void**)&f->pmid, (int64_t)D * 2}, {(void**)&f->pe, (int64_t)D * 2},
      {(void**)&f->temb, n * D * 2}, {(void**)&f->st, n * D * 2}, {(void**)&f->mods, n * (int64_t)m->NMOD * 2},
      {(void**)&f->cosT, S * 128 * 4}, {(void**)&f->sinT, S * 128 * 4}, {(void**)&f->ids, S * 3 * 4},
      {(void**)&f->tvals, (n + 1) * 4},
      {(void**)&f->xq, S * (D + SM_EXT)}, {(void**)&f->aq, S * (D + M)}, {(void**)&f->xs, S * 4}, {(void**)&f->as_, S * 4},   // 8-bit mode activations
      {(void**)&f->attn_ws, (int64_t)td_attn_streamk_ws_bytes()},
      {(void**)&f->attn8_ws, (int64_t)td_attn_fp8_ws_bytes((int)S, (int)S, cfg->num_heads)},
      {(void**)&f->href[0], (int64_t)(cfg->num_layers + cfg->num_single_layers) * cfg->num_heads * S * 4},
      {(void**)&f->href[1], (int64_t)(cfg->num_layers + cfg->num_single_layers) * cfg->num_heads * S * 4},
      {(void**)&f->hs_scale, (int64_t)(2 * cfg->num_layers + cfg->num_single_layers) * S * 4}, {(void**)&f->hs_inv, (int64_t)(2 * cfg->num_layers + cfg->num_single_layers) * S * 4},
      {(void**)&f->hs_amax, (int64_t)(2 * cfg->num_layers + cfg->num_single_layers) * S * 4},
  };
  f->hs_cap = (int)S;
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

// a fresh context on model m
int new_context(FluxModel* m, bool root, td_flux** out) {
  td_flux* f = new td_flux();
  f->m = m;
  f->root = root;
  if (int rc = alloc_workspace(f)) { delete f; return rc; }
  *out = f;
  return TD_OK;
}

constexpr size_t BC_LOG_MAX = 1 << 16;      // forwards the log keeps between two resets (a denoise loop resets it; bare forwards may go on for ever)

void block_cache_reset(td_flux* f) {
  f->bc_has_prev = false;
  f->bc_count = 0;
  f->bc_metric.clear();
  f->bc_computed.clear();
}

// The state a forward under the cache needs: buffers (first use), and values that belong to this token layout, these weights and these settings.
int block_cache_prepare(td_flux* f) {
  const FluxModel* m = f->m;
  if (!f->bc_buf) {
    const size_t rows = (size_t)m->max_img * m->D * sizeof(bf16_t);
    hipError_t e = hipMalloc((void**)&f->bc_buf, 3 * rows + TD_BLOCK_CACHE_WS_BYTES + 256);
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->bc_host, 16);
    if (e != hipSuccess) {
      td_set_error("td_flux_forward: allocating the first-block cache state (3 x %d x %d bf16) failed: %s", m->max_img, m->D, hipGetErrorString(e));
      if (f->bc_buf) (void)hipFree(f->bc_buf);
      f->bc_buf = nullptr;
      return TD_ERR_HIP;
    }
    f->bc_r[0] = (bf16_t*)f->bc_buf; f->bc_r[1] = (bf16_t*)(f->bc_buf + rows); f->bc_tail = (bf16_t*)(f->bc_buf + 2 * rows);
    f->bc_ws = (double*)(f->bc_buf + 3 * rows); f->bc_sums = (double*)(f->bc_buf + 3 * rows + TD_BLOCK_CACHE_WS_BYTES);
  }
  if (f->bc_T != f->T || f->bc_S_img != f->S_img || f->bc_S_ref != f->S_ref || f->bc_wepoch != m->weight_epoch || f->bc_cepoch != m->bc_epoch) block_cache_reset(f);
  f->bc_T = f->T; f->bc_S_img = f->S_img; f->bc_S_ref = f->S_ref; f->bc_wepoch = m->weight_epoch; f->bc_cepoch = m->bc_epoch;
  return TD_OK;
}

// Behind double block 0 (h0: the image rows before it, in f->cat): this forward's residual and metric, then the decision -- the forward's one wait
// for the device.  *skip = false: r_prev is this forward's residual and bc_tail holds h1's latent rows for block_cache_keep_tail.
int block_cache_decide(td_flux* f, hipStream_t s, bool must_compute, bool* skip) {
  const FluxModel* m = f->m;
  const int D = m->D, Si = f->S_img + f->S_ref;
  const bf16_t* h1 = f->h + (size_t)f->T * D;
  {
    TraceScope ts(f, s, TD_TRACE_NORM, 0.0);
    TD_TRY(td_block_cache_head_launch(h1, D, f->cat, D, f->bc_has_prev ? f->bc_r[f->bc_cur] : nullptr, D, f->bc_r[f->bc_cur ^ 1], D, Si, D, f->bc_sums, f->bc_ws, s));
  }
  TD_CHECK_HIP(hipMemcpyAsync(f->bc_host, f->bc_sums, 16, hipMemcpyDeviceToHost, s));
  TD_CHECK_HIP(hipStreamSynchronize(s));
  // mean |r - r_prev| / mean |r_prev| over the same element count: the ratio of the sums.  A zero denominator is "no basis to skip on".
  const double num = f->bc_host[0], den = f->bc_host[1];
  const float metric = f->bc_has_prev && den > 0.0 ? (float)(num / den) : INFINITY;
  bool compute = must_compute || !f->bc_has_prev || !(den > 0.0);
  if (!compute) {
    if (m->bc_mode == 2) compute = (size_t)f->bc_count >= m->bc_schedule.size() || m->bc_schedule[f->bc_count] != 0;
    else compute = metric > m->bc_threshold;
  }
  ++f->bc_count;
  if (f->bc_metric.size() < BC_LOG_MAX) { f->bc_metric.push_back(metric); f->bc_computed.push_back(compute ? 1 : 0); }
  *skip = !compute;
  if (compute) {
    f->bc_cur ^= 1;
    f->bc_has_prev = false;      // until block_cache_keep_tail has the tail that belongs to this residual
    TD_CHECK_HIP(hipMemcpyAsync(f->bc_tail, h1, (size_t)f->S_img * D * sizeof(bf16_t), hipMemcpyDeviceToDevice, s));
  } else {
    TraceScope ts(f, s, TD_TRACE_NORM, 0.0);
    TD_TRY(td_flux_residual_inject_launch(f->h + (size_t)f->T * D, D, f->bc_tail, D, f->S_img, D, 1.0f, s));
  }
  return TD_OK;
}

// Behind the last block of a computed forward: tail = bf16(float(h_final) - float(h1)), in place over the h1 rows
int block_cache_keep_tail(td_flux* f, hipStream_t s) {
  const int D = f->m->D;
  TraceScope ts(f, s, TD_TRACE_NORM, 0.0);
  TD_TRY(td_block_cache_tail_launch(f->h + (size_t)f->T * D, D, f->bc_tail, D, f->bc_tail, D, f->S_img, D, s));
  f->bc_has_prev = true;
  return TD_OK;
}

}  // namespace

struct FloatPack { static constexpr int N = 128; float v[N]; };
__global__ void td_set_floats_kernel(float* dst, FloatPack vals, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}

extern "C" {

int td_flux_create(const TdFluxConfig* cfg, int max_img_tokens, int max_txt_tokens, int max_steps, td_flux** out) {
  TD_CHECK_ARG(cfg && out, "td_flux_create: null argument");
  FluxModel* m = nullptr;
  TD_TRY(flux_model_create(cfg, 0, 0, max_img_tokens, max_txt_tokens, max_steps, &m));
  const int rc = new_context(m, true, out);
  if (rc != TD_OK) flux_model_destroy(m);
  return rc;
}

// A ControlNet side network ([ext] diffusers FluxControlNetModel): a second, shallower model of the same blocks with its own weights.  Its
// contexts are prepared like any (td_flux_set_condition / td_flux_set_timesteps, td_flux_fork), take the control image's latents through
// td_flux_controlnet_set_condition, and serve ONE main context each through td_flux_attach_controlnet.
int td_flux_controlnet_create(const TdFluxConfig* cfg, int num_mode, int max_img_tokens, int max_txt_tokens, int max_steps, td_flux** out) {
  TD_CHECK_ARG(cfg && out, "td_flux_controlnet_create: null argument");
  FluxModel* m = nullptr;
  TD_TRY(flux_model_create(cfg, 1, num_mode, max_img_tokens, max_txt_tokens, max_steps, &m));
  const int rc = new_context(m, true, out);
  if (rc != TD_OK) flux_model_destroy(m);
  return rc;
}

// Take ControlNet context `cn` out of main context `o`'s list: the nets behind it move up with their scale tables.
static void detach_one(td_flux* o, td_flux* cn) {
  int k = 0;
  while (k < o->n_cn && o->cns[k] != cn) ++k;
  if (k == o->n_cn) return;
  for (; k + 1 < o->n_cn; ++k) { o->cns[k] = o->cns[k + 1]; o->cn_scales[k].swap(o->cn_scales[k + 1]); }
  o->cns[--o->n_cn] = nullptr;
  o->cn_scales[o->n_cn].clear();
  cn->cn_owner = nullptr;
}

// The root context frees the model: it must outlive its forks.
void td_flux_destroy(td_flux* f) {
  if (!f) return;
  for (hipEvent_t ev : f->ev_pool) (void)hipEventDestroy(ev);
  for (int k = 0; k < f->n_cn; ++k) f->cns[k]->cn_owner = nullptr;      // either end of an attachment may go first
  if (f->cn_owner) detach_one(f->cn_owner, f);
  if (f->root) flux_model_destroy(f->m);
  for (td_flux::IpCtx& c : f->ip) if (c.buf) (void)hipFree(c.buf);
  if (f->ip_out) (void)hipFree(f->ip_out);
  if (f->bc_buf) (void)hipFree(f->bc_buf);
  if (f->bc_host) (void)hipHostFree(f->bc_host);
  (void)hipFree(f->ws);
  delete f;
}

// A second context on the same model: own workspace / conditioning / timestep schedule, so that independent images
// can be in flight on separate streams.  Precision and parameters are the model's.
int td_flux_fork(td_flux* src, td_flux** out) {
  TD_CHECK_ARG(src && out, "td_flux_fork: null argument");
  return new_context(src->m, false, out);
}

// Conditioning of one prompt: context_embedder(prompt_embeds), text_embedder(pooled), RoPE tables.
// img_ids/txt_ids are device fp32 [n,3]; txt_ids NULL = zeros (thinkdiff/models/flux_prompt.py:119).
int td_flux_set_condition(td_flux* f, const void* prompt_embeds, int T, const void* pooled, const float* txt_ids,
                          const float* img_ids, int S_img, void* stream) {
  TD_CHECK_ARG(f && prompt_embeds && pooled && img_ids, "td_flux_set_condition: null argument");
  const FluxModel* m = f->m;
  TD_CHECK_ARG(T > 0 && T <= m->max_txt && S_img > 0 && S_img <= m->max_img,
               "td_flux_set_condition: T=%d / S_img=%d exceed capacity (%d / %d)", T, S_img, m->max_txt, m->max_img);
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D;
  // A union ControlNet ([ext] controlnet_flux.py): encoder_hidden_states = cat([controlnet_mode_embedder(mode), context_embedder(enc)]) and
  // txt_ids = cat([txt_ids[:1], txt_ids]) -- its text stream has one row more than the caller's.
  const int mode_rows = m->num_mode > 0 ? 1 : 0;
  TD_CHECK_ARG(!mode_rows || f->cn_mode_id >= 0, "td_flux_set_condition: this ControlNet is a union model (num_mode=%d) and no control mode is set "
               "(td_flux_controlnet_set_mode before the condition)", m->num_mode);
  if (S_img != f->S_img) f->ccond_set = f->cn_cond_set = false;      // the channel / control condition was written for another token count
  f->S_img = S_img;
  f->S_ref = 0;      // the tables below hold T + S_img rows: reference tokens are set again after the condition, for every image
  if (mode_rows) TD_CHECK_HIP(hipMemcpyAsync(f->ctx, m->cn_mode + (size_t)f->cn_mode_id * D, (size_t)D * 2, hipMemcpyDeviceToDevice, s));
  TD_TRY(linear(f, s, m->ctx_emb, bf16_rows(prompt_embeds, m->cfg.joint_dim), T, Epilogue::to(f->ctx + (size_t)mode_rows * D, D)));
  TD_TRY(linear(f, s, m->p1, bf16_rows(pooled, m->cfg.pooled_dim), 1, Epilogue::to(f->pmid, D, TD_ACT_SILU)));
  TD_TRY(linear(f, s, m->p2, bf16_rows(f->pmid, D), 1, Epilogue::to(f->pe, D)));
  if (txt_ids) {
    if (mode_rows) TD_CHECK_HIP(hipMemcpyAsync(f->ids, txt_ids, 12, hipMemcpyDeviceToDevice, s));
    TD_CHECK_HIP(hipMemcpyAsync(f->ids + (size_t)mode_rows * 3, txt_ids, (size_t)T * 12, hipMemcpyDeviceToDevice, s));
  } else {
    TD_CHECK_HIP(hipMemsetAsync(f->ids, 0, (size_t)(T + mode_rows) * 12, s));
  }
  T += mode_rows;
  f->T = T;
  TD_CHECK_HIP(hipMemcpyAsync(f->ids + (size_t)T * 3, img_ids, (size_t)S_img * 12, hipMemcpyDeviceToDevice, s));
  TD_TRY(td_flux_rope_table_launch(f->ids, T + S_img, m->cfg.axes_dims, (double)m->cfg.rope_theta, f->cosT, f->sinT, s));
  f->cond_set = true;
  f->cond_epoch = m->weight_epoch;
  f->n_steps = 0;
  f->hs_step = f->href_step = -1;      // another image: the previous one's maxima / reference points say nothing about it
  return TD_OK;
}

// The channel condition of one image (conditioned engines): cond [S_img, Ccond] -> xin[:, Cout .. Cin), where every forward's x_embedder
// GEMM reads it beside the gathered latents.
int td_flux_set_channel_condition(td_flux* f, const void* cond, void* stream) {
  TD_CHECK_ARG(f && cond, "td_flux_set_channel_condition: null argument");
  const FluxModel* m = f->m;
  TD_CHECK_ARG(m->Ccond > 0, "td_flux_set_channel_condition: this engine takes no channel condition (in_channels = out_channels = %d)", m->Cout);
  TD_CHECK_ARG(f->cond_set, "td_flux_set_channel_condition: call td_flux_set_condition first (it fixes the image token count)");
  TD_CHECK_ARG((uintptr_t)cond % 16 == 0, "td_flux_set_channel_condition: cond must be 16-byte aligned");
  TD_TRY(td_copy_cols_launch((const bf16_t*)cond, m->Ccond, f->xin + m->Cout, m->Cin, f->S_img, m->Ccond, (hipStream_t)stream));
  f->ccond_set = true;
  f->hs_step = f->href_step = -1;      // another image, as in td_flux_set_condition: the previous one's per-token history says nothing about it
  return TD_OK;
}

// The reference tokens of one image (FLUX.1 Kontext): [ext] diffusers >= 0.34 FluxKontextPipeline.__call__
//   latent_model_input = torch.cat([latents, image_latents], dim=1);  latent_ids = torch.cat([latent_ids, image_ids], dim=0)
// ref_latents [S_ref, Cout] -> xref rows S_img ..; ref_ids [S_ref, 3] -> rows T + S_img .. of the id / RoPE tables (td_flux_rope_table's arithmetic).
int td_flux_set_reference_tokens(td_flux* f, const void* ref_latents, int S_ref, const float* ref_ids, void* stream) {
  TD_CHECK_ARG(f, "td_flux_set_reference_tokens: null context");
  const FluxModel* m = f->m;
  TD_CHECK_ARG(S_ref >= 0, "td_flux_set_reference_tokens: S_ref=%d is negative", S_ref);
  TD_CHECK_ARG(!m->controlnet, "td_flux_set_reference_tokens: S_ref=%d on a ControlNet context: a ControlNet together with reference tokens is not built", S_ref);
  TD_CHECK_ARG(m->Ccond == 0, "td_flux_set_reference_tokens: this engine is channel-conditioned (in_channels=%d, out_channels=%d); reference tokens "
               "belong to the unconditioned FLUX.1 Kontext transformer", m->Cin, m->Cout);
  TD_CHECK_ARG(f->cond_set, "td_flux_set_reference_tokens: call td_flux_set_condition first (it fixes the text and image token counts; S_ref=%d)", S_ref);
  if (S_ref == 0) {
    f->S_ref = 0;
    f->hs_step = f->href_step = -1;
    return TD_OK;
  }
  TD_CHECK_ARG(ref_latents && ref_ids, "td_flux_set_reference_tokens: null ref_latents / ref_ids with S_ref=%d", S_ref);
  TD_CHECK_ARG((long long)f->S_img + S_ref <= m->max_img, "td_flux_set_reference_tokens: S_img=%d + S_ref=%d exceed the image-stream capacity %d "
               "(max_img_tokens of td_flux_create)", f->S_img, S_ref, m->max_img);
  TD_CHECK_ARG((uintptr_t)ref_latents % 16 == 0 && (uintptr_t)ref_ids % 4 == 0, "td_flux_set_reference_tokens: ref_latents must be 16-byte, ref_ids 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const size_t row0 = (size_t)f->T + f->S_img;
  TD_CHECK_HIP(hipMemcpyAsync(f->xref + (size_t)f->S_img * m->Cout, ref_latents, (size_t)S_ref * m->Cout * 2, hipMemcpyDeviceToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(f->ids + row0 * 3, ref_ids, (size_t)S_ref * 12, hipMemcpyDeviceToDevice, s));
  TD_TRY(td_flux_rope_table_launch(f->ids + row0 * 3, S_ref, m->cfg.axes_dims, (double)m->cfg.rope_theta, f->cosT + row0 * 128, f->sinT + row0 * 128, s));
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
  TD_CHECK_ARG(f && t_eff && n > 0 && n <= f->m->max_steps, "td_flux_set_timesteps: n=%d exceeds capacity %d", n, f ? f->m->max_steps : 0);
  TD_CHECK_ARG(f->cond_set, "td_flux_set_timesteps: call td_flux_set_condition first (temb includes the pooled text embedding)");
  FluxModel* m = f->m;
  if (m->bounds_dirty) TD_TRY(flux_refresh_score_bounds(m));      // (once per weight change; set_timesteps calls are serial on the host)
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D;
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
  TD_TRY(linear(f, s, m->t1, bf16_rows(f->tproj, 256), n, Epilogue::to(f->tmid, D, TD_ACT_SILU)));
  TD_TRY(linear(f, s, m->t2, bf16_rows(f->tmid, D), n, Epilogue::to(f->te, D)));
  if (m->cfg.guidance_embeds) {
    TD_TRY(td_timestep_sincos_launch(f->tvals + n, 1, f->gproj, s));
    TD_TRY(linear(f, s, m->g1, bf16_rows(f->gproj, 256), 1, Epilogue::to(f->gmid, D, TD_ACT_SILU)));
    TD_TRY(linear(f, s, m->g2, bf16_rows(f->gmid, D), 1, Epilogue::to(f->ge, D)));
  }
  TD_TRY(td_temb_combine_silu_launch(f->te, m->cfg.guidance_embeds ? f->ge : nullptr, f->pe, n, D, f->temb, f->st, s));
  TD_TRY(linear_big_n(f, s, m->mod, bf16_rows(f->st, D), n, f->mods, m->NMOD));
  f->n_steps = n;
  f->sched_epoch = m->weight_epoch;
  f->hs_step = f->href_step = -1;      // another schedule: "the previous step" of the old one is not this one's
  return TD_OK;
}

// What the prepared context expects of its callers' buffers (the torch.ops layer validates tensor extents against it).
int td_flux_prepared_shape(const td_flux* f, int* img_tokens, int* txt_tokens, int* in_channels, int* n_steps) {
  TD_CHECK_ARG(f, "td_flux_prepared_shape: null context");
  if (img_tokens) *img_tokens = f->cond_set ? f->S_img : 0;
  if (txt_tokens) *txt_tokens = f->cond_set ? f->T : 0;
  if (in_channels) *in_channels = f->m->Cout;      // the latents' and the velocity's width (== x_embedder's on an unconditioned engine)
  if (n_steps) *n_steps = f->n_steps;
  return TD_OK;
}

int td_flux_input_shape(const td_flux* f, int* in_channels, int* cond_channels, int* cond_valid) {
  TD_CHECK_ARG(f, "td_flux_input_shape: null context");
  if (in_channels) *in_channels = f->m->Cin;
  if (cond_channels) *cond_channels = f->m->Ccond;
  if (cond_valid) *cond_valid = f->m->Ccond > 0 && f->cond_set && f->ccond_set;
  return TD_OK;
}

// What every forward asks of its context, whichever model kind it runs
static int check_prepared(const char* fn, const td_flux* f, int step) {
  TD_CHECK_ARG(f->cond_set && step >= 0 && step < f->n_steps, "%s: step %d outside the %d prepared timesteps", fn, step, f->n_steps);
  const FluxModel* m = f->m;
  TD_CHECK_ARG(f->cond_epoch == m->weight_epoch && f->sched_epoch == m->weight_epoch, "%s: weights changed since td_flux_set_condition / "
               "td_flux_set_timesteps (LoRA adapters were set, deleted or cleared; both precompute values from weights): call them again on this context", fn);
  TD_CHECK_ARG(m->Ccond == 0 || f->ccond_set, "%s: this engine reads a %d-channel condition beside the %d latent channels and none is set for "
               "the %d image tokens (td_flux_set_channel_condition after td_flux_set_condition)", fn, m->Ccond, m->Cout, f->S_img);
  return TD_OK;
}

// Called behind every block of the loop below -- (false, i): double block i, (true, i): single block i -- with the block's output in f->h.
using BlockHook = std::function<int(bool single, int i)>;

// The embedders and the block loop of BOTH model kinds on a prepared context (check_prepared), then -- velocity != null: the transformer -- the final
// AdaLayerNorm and proj_out.  A ControlNet context adds E = controlnet_x_embedder(cond) in x_embedder's epilogue and stops behind the last block;
// what it keeps of each block is its hook's business, as is what an attached ControlNet adds to the main transformer's stream.
static int run_blocks(td_flux* f, const void* latents, int step, void* velocity, const BlockHook* hook, hipStream_t s) {
  FluxModel* const m = f->m;
  const Switches sw = Switches::read();
  // Si: rows of the image stream the blocks run over (latents, then the reference tokens if any); So: the rows that are a velocity
  const int D = m->D, M = m->M, T = f->T, So = f->S_img, Si = f->S_img + f->S_ref, S = f->T + Si;
  const int H = m->cfg.num_heads, C = m->Cout;
  const int L = m->cfg.num_layers, Ls = m->cfg.num_single_layers;
  const Span txt{0, T}, img{T, Si}, all{0, S};
  const bf16_t* mod = f->mods + (size_t)step * m->NMOD;
  bf16_t* h = f->h;
  bf16_t* h_img = h + (size_t)T * D;
  const float scale = 0.08838834764831845f;  // 128^-0.5

  // ---- embed: the text rows are the condition's, the image rows x_embedder's -----------------------------------------------------
  TD_CHECK_HIP(hipMemcpyAsync(h, f->ctx, (size_t)T * D * 2, hipMemcpyDeviceToDevice, s));
  const void* x_in = latents;
  if (m->Ccond > 0) {      // Linear(cat(latents, cond)): the latents join the condition in xin, then ONE GEMM over K = Cin (one fp32 sum, one rounding)
    TD_CHECK_ARG((uintptr_t)latents % 16 == 0, "td_flux_forward: latents must be 16-byte aligned");
    TD_TRY(td_copy_cols_launch((const bf16_t*)latents, C, f->xin, m->Cin, Si, C, s));
    x_in = f->xin;
  } else if (f->S_ref > 0) {      // Linear(cat([latents, ref], dim=0)): the latents join the reference rows in xref, then ONE GEMM over all rows
    TD_CHECK_HIP(hipMemcpyAsync(f->xref, latents, (size_t)So * C * 2, hipMemcpyDeviceToDevice, s));
    x_in = f->xref;
  }
  if (m->controlnet)      // h = x_embedder(hidden) + controlnet_x_embedder(cond): each Linear rounds, then the sum (E: td_flux_controlnet_set_condition)
    TD_TRY(linear(f, s, m->x_emb, bf16_rows(x_in, m->Cin), Si, Epilogue::to(h_img, D).plus(f->cn_E, D)));
  else
    TD_TRY(linear(f, s, m->x_emb, bf16_rows(x_in, m->Cin), Si, Epilogue::to(h_img, D)));
  // first-block cache: h0 = the image rows before double block 0 (td_flux_forward prepared the state and refused what the cache does not pair with)
  const bool bc_on = m->bc_mode != 0 && velocity;
  bool bc_skip = false;
  if (bc_on) TD_CHECK_HIP(hipMemcpyAsync(f->cat, h_img, (size_t)Si * D * sizeof(bf16_t), hipMemcpyDeviceToDevice, s));

  TdNormParams np;
  np.x = h; np.ldx = D; np.y = f->xn; np.ldy = D; np.rows = S; np.D = D; np.eps = 1e-6f; np.split = T;
  TdQkRopeParams rp;
  rp.qkv = f->qkv; rp.ld = 3 * D; rp.rows = S; rp.Hq = H; rp.Hk = H; rp.q_col = 0; rp.k_col = D;
  rp.cos = f->cosT; rp.sin = f->sinT; rp.split = T; rp.eps = 1e-6f;
  rp.q_premul = scale * 1.4426950408889634f;      // q leaves RoPE in the exp2 domain of the attention kernel (one bf16 rounding, as before)
  TdAttnParams ap;
  ap.Q = f->qkv; ap.K = f->qkv + D; ap.V = f->qkv + 2 * D; ap.ldq = ap.ldkv = 3 * D;
  ap.Sq = ap.Skv = S; ap.Hq = ap.Hkv = H; ap.scale = scale; ap.batch = 1; ap.sk_ws = f->attn_ws; ap.variant = f->attn_variant | sw.attn_tune;
  ap.q_prescaled = 1;

  // 8-bit modes: the LayerNorm-modulate kernel emits quantised rows + per-token scales directly; attention / MLP outputs
  // get a per-token quantisation pass; every block Linear of a class in m8 then runs on the 8-bit MFMA path (linear / linear2 decide the same way).
  // int8 smoothing (td_flux_set_smoothing): the first forward after a change calibrates -- it runs on the bf16 path and collects channel maxima
  const bool calib = flux_calibrating(m);
  const bool sm_on = flux_smoothed(m);
  if (calib) TD_CHECK_HIP(hipMemsetAsync(m->sm_ax, 0, (size_t)m->smooth_n * 4, s));
  const unsigned m8 = flux_mask8(m);
  // 8-bit attention: its pack pass reads the raw projections and applies QK-norm + RoPE itself (bit-identical, one HBM round trip less)
  const bool rope_in_pack = m->attn_mode == TD_ATTENTION_FP8 && !sw.attn8_no_fuse;
  // 8-bit attention: every row's softmax starts from the reference its largest score of the PREVIOUS step gives (and leaves this step's for the next);
  // first steps, out-of-order steps and changed token layouts start from the first tile, as the stand-alone entry point does.
  const bool href_on = m->attn_mode == TD_ATTENTION_FP8 && !sw.attn8_no_href;
  const bool href_read = href_on && step > 0 && f->href_step == step - 1 && f->href_T == T && f->href_S == S && f->href_epoch == m->hist_epoch;
  const size_t href_blk = (size_t)H * S;
  int* const href_out = href_on ? f->href[f->href_cur ^ 1] : nullptr;
  const int* const href_in = href_read ? f->href[f->href_cur] : nullptr;
  // (href_out is cleared to 0x80808080 -- far below any reference -- block by block by the pack pass of each attention launch)
  // bf16 attention: the block's score bound as the softmax's fixed reference point (no row maxima, no rescales)
  const bool use_bound = m->attn_mode == TD_ATTENTION_BF16 && !m->bounds_dirty && !sw.attn_no_bound;
  const int q_int8 = m->precision == TD_PRECISION_INT8;
  // history scales (int8): this step quantises the MLP operands under the scales the previous step's maxima give
  const int nT = 2 * L + Ls;
  const bool hist_mode = q_int8 && m->act_scale_mode == 1 && !calib;
  const bool use_hist = hist_mode && step > 0 && f->hs_step == step - 1 && f->hs_T == T && f->hs_S == S && f->hs_epoch == m->hist_epoch;
  if (hist_mode) {
    if (use_hist) TD_TRY(td_q8_scales_from_amax_launch(f->hs_amax, f->hs_scale, f->hs_inv, (long long)nT * f->hs_cap, 1.25f, s));
    else TD_CHECK_HIP(hipMemsetAsync(f->hs_amax, 0, (size_t)nT * f->hs_cap * 4, s));
  }
  struct Hist { float *scale, *inv; unsigned* amax; };      // history tensor t (td_flux::hs_*): this step's scales, the maxima for the next
  auto hist = [&](int t) { const size_t o = (size_t)t * f->hs_cap; return Hist{f->hs_scale + o, f->hs_inv + o, f->hs_amax + o}; };
  auto attention = [&](int blk) {      // block blk of the model (double blocks first): its slice of the reference points
    return attn(f, s, ap, rope_in_pack ? &rp : nullptr, href_in ? href_in + (size_t)blk * href_blk : nullptr, href_out ? href_out + (size_t)blk * href_blk : nullptr);
  };
  // The LayerNorm ahead of Linears lA (text rows) / lB (image rows): ahead of 8-bit ones it writes quantised rows + scales -- in the smoothed form
  // divided by the Linears' factors, with their replicated channels behind the D real ones -- ahead of bf16 ones the bf16 rows
  const int DX = sm_on ? D + SM_EXT : D;
  const Rows ln{f->xn, D, f->xq, DX, f->xs};
  auto norm_for = [&](const FluxLinear& lA, const FluxLinear& lB) {
    const bool q8 = m8 & lA.cls, sm = q8 && sm_on;
    if (q8) { np.q = f->xq; np.ldq = DX; np.q_scale = f->xs; np.q_int8 = q_int8; } else { np.q = nullptr; np.q_scale = nullptr; }
    np.smoothA = sm ? m->sm_inv16 + lA.sm : nullptr; np.smoothB = sm ? m->sm_inv16 + lB.sm : nullptr;
    np.extA = sm ? m->sm_ext + (size_t)lA.ext * SM_EXT : nullptr; np.extB = sm ? m->sm_ext + (size_t)lB.ext * SM_EXT : nullptr; np.ext_n = sm ? SM_EXT : 0;
    return norm_rows(f, s, np);
  };
  // calibration: channel maxima of rows `sp` of a bf16 tensor [*, ld], K channels, into the smoothing slot `slot`
  auto cal = [&](const bf16_t* x, int ld, Span sp, int K, int64_t slot) {
    return td_col_amax_launch(x + (size_t)sp.r0 * ld, ld, sp.rows, K, m->sm_ax + slot, s);
  };

  // IP-Adapter: the slots whose image prompt this context holds (td_flux_forward vouched for them: current weights, no reference tokens, no ControlNet)
  int ip_slots[TD_IP_MAX_ADAPTERS], n_ip = 0;
  for (int a = 0; a < TD_IP_MAX_ADAPTERS; ++a) if (f->ip[a].set && m->ip[a].used) ip_slots[n_ip++] = a;

  // ---- double-stream blocks -------------------------------------------------------------------------------------------------------
  for (int i = 0; i < L; ++i) {
    const DoubleBlock& b = m->dbl[i];
    const FluxLinear* lin = b.lin;
    const bf16_t* mi = mod + (size_t)i * 12 * D;  // img: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    const bf16_t* mc = mi + 6 * D;                // ctx: same order
    // norm1 -> q | k | v
    np.shiftA = mc; np.scaleA = mc + D; np.shiftB = mi; np.scaleB = mi + D;
    TD_TRY(norm_for(lin[QKV_CTX], lin[QKV_IMG]));
    if (calib) { TD_TRY(cal(f->xn, D, txt, D, lin[QKV_CTX].sm)); TD_TRY(cal(f->xn, D, img, D, lin[QKV_IMG].sm)); }
    TD_TRY(linear2(f, s, lin[QKV_IMG], lin[QKV_CTX], ln, T, Si, Epilogue::to(f->qkv, 3 * D)));
    // IP-Adapter: ip = sum_a scale_a[i] * SDPA(norm_q(q_img), K_i^a, V_i^a) from the RAW image-row q -- here, because td_qk_norm_rope below
    // normalises AND rotates q in place (the bf16 attention mode; the e4m3 mode keeps the raw q, the position is the same in both)
    bool ip_blk = false;
    for (int j = 0; j < n_ip; ++j) {
      const td_flux::IpCtx& c = f->ip[ip_slots[j]];
      const float sc = m->ip[ip_slots[j]].scale[i];
      if (sc == 0.0f) continue;
      const bf16_t* Ki = c.kv + (size_t)(2 * i) * c.keys_pad * D;
      TraceScope ts(f, s, TD_TRACE_ATTN, 4.0 * Si * (double)c.n_keys * H * 128.0);
      TD_TRY(td_ip_attention_launch(f->qkv + (size_t)T * 3 * D, 3 * D, Ki, Ki + (size_t)c.keys_pad * D, D, f->ip_out, D, Si, H, c.n_keys, b.norm_q, 1e-6f,
                                    sc, ip_blk ? 1 : 0, s));
      ip_blk = true;
    }
    // QK-RMSNorm + RoPE -> joint attention
    rp.wqA = b.norm_added_q; rp.wkA = b.norm_added_k; rp.wqB = b.norm_q; rp.wkB = b.norm_k;
    if (!rope_in_pack) TD_TRY(qk_rope(f, s, rp));
    ap.score_bound = use_bound && (size_t)i < m->dbl_bound.size() ? m->dbl_bound[i] : 0.f;
    ap.O = f->attn; ap.ldo = D;
    // history scales: the attention epilogue writes its output as int8 under the previous step's per-token scale (the out-proj's A operand)
    const bool ao_hist = use_hist && (m8 & TD_FP8_OUT);
    const Hist ha = hist(L + Ls + i);
    if (ao_hist) { ap.q8 = f->aq; ap.ldq8 = D; ap.q8_inv = ha.inv; ap.q8_amax = ha.amax; }
    TD_TRY(attention(i));
    ap.q8 = nullptr;
    // out-projections: h += gate_msa * Linear(attention)
    if ((m8 & TD_FP8_OUT) && !ao_hist) TD_TRY(quant_act(f, s, f->attn, D, all, hist_mode ? ha.amax : nullptr));
    const Rows ao{f->attn, D, f->aq, D, ao_hist ? ha.scale : f->as_};
    TD_TRY(linear2(f, s, lin[OUT_IMG], lin[OUT_CTX], ao, T, Si, Epilogue::to(h, D).gated_residual(mi + 2 * D, mc + 2 * D)));
    // norm2 -> ff.net.0 + GELU; with history scales the intermediate leaves the epilogue as int8 as well
    np.shiftA = mc + 3 * D; np.scaleA = mc + 4 * D; np.shiftB = mi + 3 * D; np.scaleB = mi + 4 * D;
    TD_TRY(norm_for(lin[FF1_CTX], lin[FF1_IMG]));
    if (calib) { TD_TRY(cal(f->xn, D, txt, D, lin[FF1_CTX].sm)); TD_TRY(cal(f->xn, D, img, D, lin[FF1_IMG].sm)); }
    const bool ff_hist = use_hist && (m8 & TD_FP8_FF1) && (m8 & TD_FP8_FF2);
    const Hist hm = hist(i);
    Q8Out q_mlp;
    q_mlp.q = f->aq; q_mlp.ld = M; q_mlp.inv = hm.inv; q_mlp.amax = hm.amax;
    if (sm_on) { q_mlp.smooth = m->sm_inv16 + lin[FF2_IMG].sm; q_mlp.smooth_ctx = m->sm_inv16 + lin[FF2_CTX].sm; }
    TD_TRY(linear2(f, s, lin[FF1_IMG], lin[FF1_CTX], ln, T, Si, Epilogue::to(f->mlp, M, TD_ACT_GELU_TANH).int8_out(ff_hist ? &q_mlp : nullptr)));
    if (calib) { TD_TRY(cal(f->mlp, M, txt, M, lin[FF2_CTX].sm)); TD_TRY(cal(f->mlp, M, img, M, lin[FF2_IMG].sm)); }
    // ff.net.2: h += gate_mlp * Linear(intermediate)
    if ((m8 & TD_FP8_FF2) && !ff_hist) {
      if (sm_on) {      // the two streams meet different weights: their own factors
        TD_TRY(quant_act(f, s, f->mlp, M, txt, hist_mode ? hm.amax : nullptr, m->sm_inv + lin[FF2_CTX].sm));
        TD_TRY(quant_act(f, s, f->mlp, M, img, hist_mode ? hm.amax : nullptr, m->sm_inv + lin[FF2_IMG].sm));
      } else {
        TD_TRY(quant_act(f, s, f->mlp, M, all, hist_mode ? hm.amax : nullptr));
      }
    }
    const Rows mo{f->mlp, M, f->aq, M, ff_hist ? hm.scale : f->as_};
    TD_TRY(linear2(f, s, lin[FF2_IMG], lin[FF2_CTX], mo, T, Si, Epilogue::to(h, D).gated_residual(mi + 5 * D, mc + 5 * D)));
    if (ip_blk) {      // hidden = hidden + ip: one bf16 add behind the gated FF residual (scale 1.0: bf16(1.0 x ip) is ip)
      TraceScope ts(f, s, TD_TRACE_NORM, 0.0);
      TD_TRY(td_flux_residual_inject_launch(h_img, D, f->ip_out, D, Si, D, 1.0f, s));
    }
    if (hook) TD_TRY((*hook)(false, i));
    if (bc_on && i == 0) {      // (a pending calibration must see every block)
      TD_TRY(block_cache_decide(f, s, calib, &bc_skip));
      if (bc_skip) break;
    }
  }

  // ---- single-stream blocks -------------------------------------------------------------------------------------------------------
  for (int i = 0; i < Ls && !bc_skip; ++i) {
    const SingleBlock& b = m->sgl[i];
    const FluxLinear &w1 = b.lin[SINGLE_IN], &w2 = b.lin[SINGLE_OUT];
    const bf16_t* ms = mod + (size_t)L * 12 * D + (size_t)i * 3 * D;  // shift, scale, gate
    // norm -> q | k | v into qkv, GELU(proj_mlp) into the MLP half of [attn | mlp] (one launch, split output)
    np.shiftA = np.shiftB = ms; np.scaleA = np.scaleB = ms + D;
    TD_TRY(norm_for(w1, w1));
    if (calib) TD_TRY(cal(f->xn, D, all, D, w1.sm));
    const bool sg_hist = use_hist && (m8 & TD_FP8_SINGLE_IN) && (m8 & TD_FP8_SINGLE_OUT);
    const Hist hc = hist(L + i);
    Q8Out q_mlp;
    q_mlp.q = f->aq + D; q_mlp.ld = D + M; q_mlp.inv = hc.inv; q_mlp.amax = hc.amax;      // the mlp half of [attn | mlp], int8, straight from the epilogue
    if (sm_on) q_mlp.smooth = m->sm_inv16 + w2.sm + D - 3 * D;      // indexed by the launch's absolute output column n >= 3 D: w2's MLP channels start at w2.sm + D
    TD_TRY(linear(f, s, w1, ln, S, Epilogue::to(f->qkv, 3 * D).split(3 * D, f->cat + D, D + M, TD_ACT_GELU_TANH).int8_out(sg_hist ? &q_mlp : nullptr)));
    if (calib) TD_TRY(cal(f->cat + D, D + M, all, M, w2.sm + D));
    // QK-RMSNorm + RoPE -> attention into the other half
    rp.wqA = rp.wqB = b.norm_q; rp.wkA = rp.wkB = b.norm_k;
    if (!rope_in_pack) TD_TRY(qk_rope(f, s, rp));
    ap.score_bound = use_bound && (size_t)i < m->sgl_bound.size() ? m->sgl_bound[i] : 0.f;
    ap.O = f->cat; ap.ldo = D + M;
    if (sg_hist) { ap.q8 = f->aq; ap.ldq8 = D + M; ap.q8_inv = hc.inv; ap.q8_amax = hc.amax; }   // the attention half of [attn | mlp] as int8, same per-token scale
    TD_TRY(attention(L + i));
    ap.q8 = nullptr;
    // proj_out: h += gate * Linear([attn | mlp]); under sg_hist both halves of the operand are in f->aq already (the two epilogues above)
    if ((m8 & TD_FP8_SINGLE_OUT) && !sg_hist)
      TD_TRY(quant_act(f, s, f->cat, D + M, all, hist_mode ? hc.amax : nullptr, sm_on ? m->sm_inv + w2.sm : nullptr));
    const Rows co{f->cat, D + M, f->aq, D + M, sg_hist ? hc.scale : f->as_};
    TD_TRY(linear(f, s, w2, co, S, Epilogue::to(h, D).gated_residual(ms + 2 * D)));
    if (hook) TD_TRY((*hook)(true, i));
  }

  // ---- AdaLayerNormContinuous (chunk order: scale, shift) and proj_out, on the latents' image rows only (reference tokens have no velocity)
  if (bc_on && !bc_skip) TD_TRY(block_cache_keep_tail(f, s));
  if (velocity) {
    const bf16_t* mf = mod + (size_t)L * 12 * D + (size_t)Ls * 3 * D;
    TdNormParams nf = np;
    nf.q = nullptr;   // the final projection stays bf16
    nf.smoothA = nf.smoothB = nullptr; nf.extA = nf.extB = nullptr; nf.ext_n = 0;
    nf.x = h_img; nf.y = f->xn; nf.rows = So; nf.split = 0;
    nf.scaleA = nf.scaleB = mf; nf.shiftA = nf.shiftB = mf + D;
    TD_TRY(norm_rows(f, s, nf));
    TD_TRY(linear(f, s, m->proj, bf16_rows(f->xn, D), So, Epilogue::to((bf16_t*)velocity, C)));
  }
  if (calib) TD_TRY(flux_finish_smoothing(m, s));      // (synchronises s; bumps the history epoch)
  if (hist_mode) { f->hs_step = step; f->hs_T = T; f->hs_S = S; f->hs_epoch = m->hist_epoch; } else f->hs_step = -1;
  if (href_on) { f->href_cur ^= 1; f->href_step = step; f->href_T = T; f->href_S = S; f->href_epoch = m->hist_epoch; } else f->href_step = -1;
  if (bc_skip) f->hs_step = f->href_step = -1;      // only block 0 left maxima / reference points: the next forward starts afresh, as after an out-of-order step
  return TD_OK;
}

// sample k of a ControlNet context's arena (double-block samples first)
static bf16_t* cn_sample(const td_flux* cn, int k) { return cn->cn_samples + (size_t)k * cn->m->max_img * cn->m->D; }

// One ControlNet evaluation on its own context: behind block i the i-th output Linear runs from the image rows into the sample arena, UNSCALED
// (controlnet_blocks[i](block_sample[i]), controlnet_single_blocks[i](single_sample[i])); the conditioning scale meets them where they are injected.
static int controlnet_forward(const char* fn, td_flux* cn, const void* latents, int step, hipStream_t s) {
  TD_TRY(check_prepared(fn, cn, step));
  TD_CHECK_ARG(cn->cn_cond_set, "%s: the ControlNet context holds no control condition for its %d image tokens (td_flux_controlnet_set_condition after "
               "td_flux_set_condition)", fn, cn->S_img);
  const FluxModel* m = cn->m;
  const int D = m->D, L = m->cfg.num_layers;
  const bf16_t* h_img = cn->h + (size_t)cn->T * D;
  const BlockHook keep = [&](bool single, int i) {
    const FluxLinear& l = single ? m->cn_sgl[i] : m->cn_dbl[i];
    return linear(cn, s, l, bf16_rows(h_img, D), cn->S_img, Epilogue::to(cn_sample(cn, single ? L + i : i), D));
  };
  return run_blocks(cn, latents, step, nullptr, &keep, s);
}

int td_flux_controlnet_forward(td_flux* cn, const void* latents, int step, void* stream) {
  TD_CHECK_ARG(cn && latents, "td_flux_controlnet_forward: null argument");
  TD_CHECK_ARG(cn->m->controlnet, "td_flux_controlnet_forward: not a ControlNet context (td_flux_controlnet_create makes one)");
  return controlnet_forward("td_flux_controlnet_forward", cn, latents, step, (hipStream_t)stream);
}

// One transformer evaluation: velocity[S_img, out_channels] = FluxTransformer2DModel(latents; step).  With a ControlNet context attached and a
// non-zero conditioning scale at this step ([ext] diffusers FluxControlNetPipeline's loop body): first the ControlNet on the same latents, step
// and stream, then the blocks with   hidden = hidden + bf16(scale * sample[i / ceil(n_blocks / n_samples)])   behind each, image rows only.
// With several attached (td_flux_attach_controlnets) the nets whose scale is not 0 run one after another and ONE launch behind each block adds the
// bf16 left fold of their scaled samples (td_flux_residual_inject_multi_bf16).  With nothing attached, or every scale 0 (h + 0 is h), exactly the
// launches of the plain forward.
int td_flux_forward(td_flux* f, const void* latents, int step, void* velocity, void* stream) {
  TD_CHECK_ARG(f && latents && velocity, "td_flux_forward: null argument");
  FluxModel* const m = f->m;
  TD_CHECK_ARG(!m->controlnet, "td_flux_forward: a ControlNet context has no velocity (td_flux_controlnet_forward runs it; td_flux_attach_controlnet makes a "
               "main context run it)");
  TD_TRY(check_prepared("td_flux_forward", f, step));
  for (int a = 0; a < TD_IP_MAX_ADAPTERS; ++a) {
    if (!f->ip[a].set) continue;
    TD_CHECK_ARG(m->ip[a].used && f->ip[a].epoch == m->ip[a].epoch, "td_flux_forward: the weights of IP-Adapter slot %d changed since td_flux_set_ip_image_embeds on this "
                 "context (td_flux_ip_adapter_load_param / _remove; its K / V are values of the old ones): set the image embeds again, or clear them", a);
    TD_CHECK_ARG(f->S_ref == 0, "td_flux_forward: IP-Adapter slot %d holds an image prompt and the context %d reference tokens (the image rows would include "
                 "the reference rows): that pairing is not built", a, f->S_ref);
    TD_CHECK_ARG(f->n_cn == 0, "td_flux_forward: IP-Adapter slot %d holds an image prompt and a ControlNet is attached: that pairing is not built", a);
  }
  if (m->bc_mode != 0) {
    TD_CHECK_ARG(f->n_cn == 0, "td_flux_forward: the first-block cache is on (mode %d) and a ControlNet is attached (its samples are added behind every block, "
                 "a skipped forward runs one): that pairing is not built", m->bc_mode);
    TD_CHECK_ARG(m->cfg.num_layers > 0, "td_flux_forward: the first-block cache is on (mode %d) and the model has no double-stream block to decide behind", m->bc_mode);
    TD_TRY(block_cache_prepare(f));
  }
  hipStream_t s = (hipStream_t)stream;
  // the nets that take part in this step, in list order: scale != 0 (a net at scale 0 is neither run nor folded)
  td_flux* act[TD_MAX_CONTROLNETS];
  float sc[TD_MAX_CONTROLNETS];
  int idx[TD_MAX_CONTROLNETS], n_act = 0;
  for (int k = 0; k < f->n_cn; ++k) {
    const float v = (size_t)step < f->cn_scales[k].size() ? f->cn_scales[k][step] : 1.0f;
    if (v == 0.0f) continue;
    td_flux* const cn = f->cns[k];
    const FluxModel* c = cn->m;
    TD_CHECK_ARG(c->D == m->D && c->cfg.num_heads == m->cfg.num_heads, "td_flux_forward: the attached ControlNet %d has inner width %d (%d heads), the transformer "
                 "%d (%d heads)", k, c->D, c->cfg.num_heads, m->D, m->cfg.num_heads);
    TD_CHECK_ARG(m->Ccond == 0, "td_flux_forward: a ControlNet (%d) is attached to a channel-conditioned transformer (in_channels=%d, out_channels=%d): that pairing "
                 "is not built", k, m->Cin, m->Cout);
    TD_CHECK_ARG(c->Cin == m->Cout, "td_flux_forward: the attached ControlNet %d reads %d latent channels, the transformer steps %d", k, c->Cin, m->Cout);
    TD_CHECK_ARG(f->S_ref == 0, "td_flux_forward: a ControlNet (%d) is attached and the context holds %d reference tokens: a ControlNet together with reference "
                 "tokens is not built", k, f->S_ref);
    TD_CHECK_ARG(cn->cond_set && cn->S_img == f->S_img, "td_flux_forward: the attached ControlNet context %d is prepared for %d image tokens, this context for %d "
                 "(td_flux_set_condition on both, per image)", k, cn->cond_set ? cn->S_img : 0, f->S_img);
    TD_CHECK_ARG(cn->n_steps == f->n_steps, "td_flux_forward: the attached ControlNet context %d is prepared for %d timesteps, this context for %d", k, cn->n_steps,
                 f->n_steps);
    act[n_act] = cn; sc[n_act] = v; idx[n_act++] = k;
  }
  if (n_act == 0) return run_blocks(f, latents, step, velocity, nullptr, s);
  for (int a = 0; a < n_act; ++a) {      // one after another on the same latents, step and stream; each into its own arena
    char fn[64];
    snprintf(fn, sizeof(fn), "td_flux_forward(attached ControlNet %d)", idx[a]);
    act[a]->attn_variant = f->attn_variant; act[a]->shared_chip = f->shared_chip;      // images in flight: the side network's kernels follow its image's
    TD_TRY(controlnet_forward(fn, act[a], latents, step, s));
  }
  // behind block i: net a's sample i / ceil(n_blocks / n_samples_a) -- every net by ITS OWN counts; trailing samples may stay unused, and a net
  // without single blocks takes no part behind the single blocks.  One launch over the nets that take part (one net: the single-net kernel).
  const int D = m->D, L = m->cfg.num_layers, Ls = m->cfg.num_single_layers;
  bf16_t* h_img = f->h + (size_t)f->T * D;
  const BlockHook inject = [&](bool single, int i) {
    const bf16_t* r[TD_MAX_CONTROLNETS];
    int ld[TD_MAX_CONTROLNETS], n = 0;
    float w[TD_MAX_CONTROLNETS];
    for (int a = 0; a < n_act; ++a) {
      const int nd = act[a]->m->cfg.num_layers, ns = act[a]->m->cfg.num_single_layers;
      if (single && ns == 0) continue;
      const int per = single ? (Ls + ns - 1) / ns : (L + nd - 1) / nd;
      r[n] = cn_sample(act[a], single ? nd + i / per : i / per); ld[n] = D; w[n++] = sc[a];
    }
    if (n == 0) return (int)TD_OK;
    TraceScope ts(f, s, TD_TRACE_NORM, 0.0);
    if (n == 1) return td_flux_residual_inject_launch(h_img, D, r[0], D, f->S_img, D, w[0], s);
    return td_flux_residual_inject_multi_launch(h_img, D, r, ld, w, n, f->S_img, D, s);
  };
  return run_blocks(f, latents, step, velocity, &inject, s);
}

// The control mode of a union ControlNet (row of controlnet_mode_embedder the next td_flux_set_condition prepends); -1 clears.
int td_flux_controlnet_set_mode(td_flux* cn, int mode) {
  TD_CHECK_ARG(cn, "td_flux_controlnet_set_mode: null context");
  TD_CHECK_ARG(cn->m->controlnet, "td_flux_controlnet_set_mode: not a ControlNet context");
  TD_CHECK_ARG(mode == -1 || cn->m->num_mode > 0, "td_flux_controlnet_set_mode: mode %d on a ControlNet without a mode embedder (num_mode = 0)", mode);
  TD_CHECK_ARG(mode >= -1 && mode < cn->m->num_mode, "td_flux_controlnet_set_mode: mode %d outside the %d rows of controlnet_mode_embedder", mode, cn->m->num_mode);
  if (mode != cn->cn_mode_id) cn->cond_set = false;      // the text stream's first row is another: the condition must be set again
  cn->cn_mode_id = mode;
  return TD_OK;
}

// The control image of one image: control_latents bf16 [S_img, in_channels] (packed, shifted / scaled) -> E = controlnet_x_embedder(cond), once;
// every forward of the context then adds E in x_embedder's epilogue.
int td_flux_controlnet_set_condition(td_flux* cn, const void* control_latents, void* stream) {
  TD_CHECK_ARG(cn && control_latents, "td_flux_controlnet_set_condition: null argument");
  const FluxModel* m = cn->m;
  TD_CHECK_ARG(m->controlnet, "td_flux_controlnet_set_condition: not a ControlNet context");
  TD_CHECK_ARG(cn->cond_set, "td_flux_controlnet_set_condition: call td_flux_set_condition first (it fixes the image token count)");
  TD_CHECK_ARG((uintptr_t)control_latents % 16 == 0, "td_flux_controlnet_set_condition: control_latents must be 16-byte aligned");
  TD_TRY(linear(cn, (hipStream_t)stream, m->cn_x_emb, bf16_rows(control_latents, m->Cin), cn->S_img, Epilogue::to(cn->cn_E, m->D)));
  cn->cn_cond_set = true;
  return TD_OK;
}

int td_flux_controlnet_samples(const td_flux* cn, void** base, int* n_double, int* n_single, int64_t* stride_elems, int* rows, int* width) {
  TD_CHECK_ARG(cn, "td_flux_controlnet_samples: null context");
  TD_CHECK_ARG(cn->m->controlnet, "td_flux_controlnet_samples: not a ControlNet context");
  if (base) *base = cn->cn_samples;
  if (n_double) *n_double = cn->m->cfg.num_layers;
  if (n_single) *n_single = cn->m->cfg.num_single_layers;
  if (stride_elems) *stride_elems = (int64_t)cn->m->max_img * cn->m->D;
  if (rows) *rows = cn->cond_set ? cn->S_img : 0;
  if (width) *width = cn->m->D;
  return TD_OK;
}

// sample k of the last forward -> dst bf16 [rows, width] contiguous (one device-to-device copy on `stream`)
int td_flux_controlnet_read_sample(const td_flux* cn, int k, void* dst, void* stream) {
  TD_CHECK_ARG(cn && dst, "td_flux_controlnet_read_sample: null argument");
  TD_CHECK_ARG(cn->m->controlnet && cn->cond_set, "td_flux_controlnet_read_sample: a prepared ControlNet context is required");
  const int n = cn->m->cfg.num_layers + cn->m->cfg.num_single_layers;
  TD_CHECK_ARG(k >= 0 && k < n, "td_flux_controlnet_read_sample: sample %d outside the %d the model produces", k, n);
  TD_CHECK_HIP(hipMemcpyAsync(dst, cn_sample(cn, k), (size_t)cn->S_img * cn->m->D * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

// ControlNet contexts cns[0 .. n) onto main context f, in list order; n = 0 detaches all.  One main context per ControlNet context.  Every scale
// table returns to 1.0.  Nothing changes when a check fails.
static int attach_controlnets(const char* fn, td_flux* f, td_flux* const* cns, int n) {
  TD_CHECK_ARG(f, "%s: null context", fn);
  TD_CHECK_ARG(n >= 0 && n <= TD_MAX_CONTROLNETS, "%s: n=%d ControlNets outside 0 .. %d", fn, n, TD_MAX_CONTROLNETS);
  TD_CHECK_ARG(n == 0 || cns, "%s: null list of %d ControlNet contexts", fn, n);
  for (int k = 0; k < n; ++k) {      // (the list itself first: no context is looked into before the list is sound)
    TD_CHECK_ARG(cns[k], "%s: ControlNet context %d of %d is null", fn, k, n);
    for (int j = 0; j < k; ++j)
      TD_CHECK_ARG(cns[j] != cns[k], "%s: entries %d and %d are the same ControlNet context (each holds ONE mode, condition and sample arena: list a "
                   "fork of it instead)", fn, j, k);
  }
  TD_CHECK_ARG(!f->m->controlnet, "%s: the first argument is a ControlNet context (attach a ControlNet TO a transformer context)", fn);
  for (int k = 0; k < n; ++k) {
    td_flux* const cn = cns[k];
    TD_CHECK_ARG(cn->m->controlnet, "%s: the second argument is not a ControlNet context (entry %d; td_flux_controlnet_create makes one)", fn, k);
    TD_CHECK_ARG(!cn->cn_owner || cn->cn_owner == f, "%s: this ControlNet context (entry %d) already serves another main context (one at a time: "
                 "fork the ControlNet, one fork per main context)", fn, k);
  }
  for (int k = 0; k < f->n_cn; ++k) { f->cns[k]->cn_owner = nullptr; f->cns[k] = nullptr; }
  for (int k = 0; k < TD_MAX_CONTROLNETS; ++k) f->cn_scales[k].clear();
  for (int k = 0; k < n; ++k) { f->cns[k] = cns[k]; cns[k]->cn_owner = f; }
  f->n_cn = n;
  return TD_OK;
}

int td_flux_attach_controlnets(td_flux* f, td_flux* const* cns, int n) { return attach_controlnets("td_flux_attach_controlnets", f, cns, n); }

// the n = 1 form; cn == NULL: the n = 0 form
int td_flux_attach_controlnet(td_flux* f, td_flux* cn) { return attach_controlnets("td_flux_attach_controlnet", f, &cn, cn ? 1 : 0); }

int td_flux_attached_controlnets(const td_flux* f, int* n) {
  TD_CHECK_ARG(f && n, "td_flux_attached_controlnets: null argument");
  *n = f->n_cn;
  return TD_OK;
}

// net k's conditioning scale of every prepared step (host floats; diffusers: controlnet_conditioning_scale[k] x controlnet_keep[i][k]); steps beyond n keep 1.0
static int set_controlnet_scales(const char* fn, td_flux* f, int k, const float* scales, int n) {
  TD_CHECK_ARG(f && n >= 0 && (n == 0 || scales), "%s: null argument", fn);
  TD_CHECK_ARG(k >= 0 && k < TD_MAX_CONTROLNETS, "%s: ControlNet %d outside 0 .. %d", fn, k, TD_MAX_CONTROLNETS - 1);
  TD_CHECK_ARG(!f->m->controlnet, "%s: the scales belong to the main context the ControlNet is attached to", fn);
  TD_CHECK_ARG(f->n_cn > 0, "%s: no ControlNet is attached (td_flux_attach_controlnet)", fn);
  TD_CHECK_ARG(k < f->n_cn, "%s: ControlNet %d outside the %d attached", fn, k, f->n_cn);
  TD_CHECK_ARG(n <= f->m->max_steps, "%s: n=%d exceeds the %d steps of capacity", fn, n, f->m->max_steps);
  for (int i = 0; i < n; ++i) TD_CHECK_ARG(std::isfinite(scales[i]), "%s: scale %d is not finite", fn, i);
  f->cn_scales[k].assign(scales, scales + n);
  return TD_OK;
}

int td_flux_set_controlnet_scales(td_flux* f, const float* scales, int n) { return set_controlnet_scales("td_flux_set_controlnet_scales", f, 0, scales, n); }

int td_flux_set_controlnet_scales_at(td_flux* f, int k, const float* scales, int n) {
  return set_controlnet_scales("td_flux_set_controlnet_scales_at", f, k, scales, n);
}

// The image prompt of one image for IP-Adapter slot `slot` on THIS context (include/thinkdiff_hip.h spells the arithmetic): the projection and the
// 2 L K / V Linears, once; every forward of the context then reads the arena.  NULL clears.
int td_flux_set_ip_image_embeds(td_flux* f, int slot, const void* embeds, int n_img, void* stream) {
  TD_CHECK_ARG(f, "td_flux_set_ip_image_embeds: null context");
  TD_CHECK_ARG(slot >= 0 && slot < TD_IP_MAX_ADAPTERS, "td_flux_set_ip_image_embeds: slot %d outside 0 .. %d", slot, TD_IP_MAX_ADAPTERS - 1);
  td_flux::IpCtx& c = f->ip[slot];
  if (!embeds) { c.set = false; return TD_OK; }
  FluxModel* const m = f->m;
  TD_CHECK_ARG(!m->controlnet, "td_flux_set_ip_image_embeds: a ControlNet context takes no image prompt");
  const IpAdapter& a = m->ip[slot];
  TD_CHECK_ARG(a.used, "td_flux_set_ip_image_embeds: slot %d holds no adapter (td_flux_ip_adapter_add)", slot);
  for (const auto& kv : a.params)
    TD_CHECK_ARG(kv.second.loaded, "td_flux_set_ip_image_embeds: parameter '%s' of slot %d is not loaded (td_flux_ip_adapter_load_param)", kv.first.c_str(), slot);
  TD_CHECK_ARG(n_img >= 1, "td_flux_set_ip_image_embeds: n_img=%d", n_img);
  TD_CHECK_ARG((long long)n_img * a.num_tokens <= TD_IP_MAX_KEYS, "td_flux_set_ip_image_embeds: %d images x %d tokens = %lld keys exceed TD_IP_MAX_KEYS = %d", n_img,
               a.num_tokens, (long long)n_img * a.num_tokens, TD_IP_MAX_KEYS);
  TD_CHECK_ARG((uintptr_t)embeds % 16 == 0, "td_flux_set_ip_image_embeds: embeds must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t J = m->cfg.joint_dim, D = m->D, L = m->cfg.num_layers;
  const int n_keys = n_img * a.num_tokens, keys_pad = (n_keys + 31) & ~31;
  auto up = [](int64_t b) { return (b + 255) & ~int64_t(255); };
  const int64_t b_stage = up((int64_t)n_img * a.E_pad * 2), b_proj = up((int64_t)n_keys * J * 2), b_kv = up(L * 2 * keys_pad * D * 2);
  const int64_t need = b_stage + 2 * b_proj + b_kv;
  c.set = false;
  if (need > c.bytes) {      // first use, or more keys than before (hipFree waits for the device: nobody reads the old arena any more)
    if (c.buf) (void)hipFree(c.buf);
    c.buf = nullptr; c.bytes = 0;
    hipError_t e = hipMalloc((void**)&c.buf, (size_t)need);
    if (e != hipSuccess) {
      td_set_error("td_flux_set_ip_image_embeds: hipMalloc of %.1f MiB for slot %d failed: %s", need / double(1 << 20), slot, hipGetErrorString(e));
      return TD_ERR_HIP;
    }
    c.bytes = need;
  }
  if (!f->ip_out) {
    hipError_t e = hipMalloc((void**)&f->ip_out, (size_t)m->max_img * D * 2);
    if (e != hipSuccess) {
      td_set_error("td_flux_set_ip_image_embeds: hipMalloc of the %d x %lld output buffer failed: %s", m->max_img, (long long)D, hipGetErrorString(e));
      return TD_ERR_HIP;
    }
  }
  c.stage = (bf16_t*)c.buf; c.projd = (bf16_t*)(c.buf + b_stage); c.tokens = (bf16_t*)(c.buf + b_stage + b_proj); c.kv = (bf16_t*)(c.buf + b_stage + 2 * b_proj);
  c.n_img = n_img; c.n_keys = n_keys; c.keys_pad = keys_pad;
  // embeds -> rows of E_pad (zeros behind E), then tokens = LayerNorm_J(proj(embeds).reshape(n_keys, J))
  TD_CHECK_HIP(hipMemsetAsync(c.stage, 0, (size_t)b_stage, s));
  TD_CHECK_HIP(hipMemcpy2DAsync(c.stage, (size_t)a.E_pad * 2, embeds, (size_t)a.E * 2, (size_t)a.E * 2, (size_t)n_img, hipMemcpyDeviceToDevice, s));
  auto par = [&](const std::string& name) { return a.params.at(name).ptr; };
  FluxLinear proj;
  proj.w = par("image_proj.proj.weight"); proj.b = par("image_proj.proj.bias"); proj.N = (int)(a.num_tokens * J); proj.K = a.E_pad;
  TD_TRY(linear(f, s, proj, bf16_rows(c.stage, a.E_pad), n_img, Epilogue::to(c.projd, proj.N)));
  TD_TRY(td_norm_rows_generic_launch(c.projd, (int)J, c.tokens, (int)J, n_keys, (int)J, 0, 1e-5f, par("image_proj.norm.weight"), par("image_proj.norm.bias"), s));
  TD_CHECK_HIP(hipMemsetAsync(c.kv, 0, (size_t)b_kv, s));
  for (int i = 0; i < L; ++i)
    for (int w = 0; w < 2; ++w) {
      const std::string base = "ip_adapter." + std::to_string(i) + (w ? ".to_v_ip" : ".to_k_ip");
      FluxLinear l;
      l.w = par(base + ".weight"); l.b = par(base + ".bias"); l.N = (int)D; l.K = (int)J;
      TD_TRY(linear(f, s, l, bf16_rows(c.tokens, (int)J), n_keys, Epilogue::to(c.kv + (size_t)(2 * i + w) * keys_pad * D, (int)D)));
    }
  c.epoch = a.epoch;
  c.set = true;
  return TD_OK;
}

int td_flux_ip_read(const td_flux* f, int slot, int block, int which, void* dst, void* stream) {
  TD_CHECK_ARG(f && dst && slot >= 0 && slot < TD_IP_MAX_ADAPTERS, "td_flux_ip_read: null argument or slot %d outside 0 .. %d", slot, TD_IP_MAX_ADAPTERS - 1);
  const td_flux::IpCtx& c = f->ip[slot];
  TD_CHECK_ARG(c.set, "td_flux_ip_read: slot %d holds no image prompt on this context", slot);
  const FluxModel* m = f->m;
  TD_CHECK_ARG(block < m->cfg.num_layers && (which == 0 || which == 1), "td_flux_ip_read: block %d of %d, which=%d (0 = K, 1 = V)", block, m->cfg.num_layers, which);
  const bf16_t* src = block < 0 ? c.tokens : c.kv + (size_t)(2 * block + which) * c.keys_pad * m->D;
  const size_t width = block < 0 ? (size_t)m->cfg.joint_dim : (size_t)m->D;
  TD_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)c.n_keys * width * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

int td_flux_ip_widths(const td_flux* f, int* joint_dim, int* inner_dim) {
  TD_CHECK_ARG(f, "td_flux_ip_widths: null context");
  if (joint_dim) *joint_dim = f->m->cfg.joint_dim;
  if (inner_dim) *inner_dim = f->m->D;
  return TD_OK;
}

// First-block cache, the model's settings (include/thinkdiff_hip.h spells the semantics).  Every change voids every context's state (bc_epoch).
static int block_cache_model(const char* fn, td_flux* f, int mode) {
  TD_CHECK_ARG(f, "%s: null context", fn);
  TD_CHECK_ARG(f->root, "%s: mode %d asked of a fork: the cache settings are the model's (call it on the parent context; forks follow)", fn, mode);
  TD_CHECK_ARG(!f->m->controlnet, "%s: mode %d asked of a ControlNet model: it has no velocity to cache, and a transformer with a ControlNet attached refuses "
               "the cache as well", fn, mode);
  return TD_OK;
}

int td_flux_set_block_cache(td_flux* f, int mode, float threshold) {
  TD_TRY(block_cache_model("td_flux_set_block_cache", f, mode));
  TD_CHECK_ARG(mode == 0 || mode == 1, "td_flux_set_block_cache: mode %d (0 = off, 1 = threshold; td_flux_set_block_cache_schedule sets mode 2)", mode);
  TD_CHECK_ARG(mode == 0 || threshold >= 0.0f, "td_flux_set_block_cache: threshold %g must be a number >= 0 (0 = always compute)", (double)threshold);
  FluxModel* m = f->m;
  m->bc_mode = mode;
  m->bc_threshold = mode ? threshold : 0.f;
  m->bc_schedule.clear();
  ++m->bc_epoch;
  return TD_OK;
}

int td_flux_set_block_cache_schedule(td_flux* f, const unsigned char* compute, int n) {
  TD_TRY(block_cache_model("td_flux_set_block_cache_schedule", f, 2));
  TD_CHECK_ARG(compute && n > 0, "td_flux_set_block_cache_schedule: an empty schedule (n=%d)", n);
  TD_CHECK_ARG(compute[0] != 0, "td_flux_set_block_cache_schedule: the schedule of %d forwards starts with a skip: the first forward has nothing to reuse", n);
  FluxModel* m = f->m;
  m->bc_mode = 2;
  m->bc_threshold = 0.f;
  m->bc_schedule.assign(compute, compute + n);
  ++m->bc_epoch;
  return TD_OK;
}

int td_flux_block_cache_reset(td_flux* f) {
  TD_CHECK_ARG(f, "td_flux_block_cache_reset: null context");
  block_cache_reset(f);
  return TD_OK;
}

int td_flux_block_cache_stats(const td_flux* f, int cap, float* metric, unsigned char* computed, int* n) {
  TD_CHECK_ARG(f && n && cap >= 0 && (cap == 0 || (metric && computed)), "td_flux_block_cache_stats: null argument (cap=%d)", cap);
  *n = (int)f->bc_metric.size();
  for (int i = 0; i < cap && i < *n; ++i) { metric[i] = f->bc_metric[i]; computed[i] = f->bc_computed[i]; }
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
  const size_t bytes = (size_t)fs[k]->S_img * fs[k]->m->Cout * sizeof(bf16_t);
  const void* bufs[3] = {b.z, b.noise, b.mask};
  static const char* names[3] = {"image_latents", "noise", "mask"};
  for (int j = 0; j < 3; ++j) {
    TD_CHECK_ARG((uintptr_t)bufs[j] % 16 == 0, "%s: image %d: %s must be 16-byte aligned", fn, k, names[j]);
    for (int l = 0; l < count; ++l)
      TD_CHECK_ARG(!overlaps(bufs[j], bytes, latents[l], (size_t)fs[l]->S_img * fs[l]->m->Cout * sizeof(bf16_t)),
                   "%s: image %d: %s overlaps the latents of image %d (the loop writes them in place)", fn, k, names[j], l);
  }
  return TD_OK;
}

// the scheduler step of loop step i (of n) after the forward wrote f->vout: Euler, or Euler + scale_noise + mask blend
int scheduler_step(td_flux* f, void* latents, const float* sigmas, int i, int n, const InpaintBlend* b, void* stream) {
  const long long count = (long long)f->S_img * f->m->Cout;
  if (!b) return td_euler_step_launch((bf16_t*)latents, f->vout, sigmas[i + 1] - sigmas[i], count, (hipStream_t)stream);
  return td_flux_inpaint_step_launch((bf16_t*)latents, f->vout, (const bf16_t*)b->z, i < n - 1 ? (const bf16_t*)b->noise : nullptr,
                                     (const bf16_t*)b->mask, sigmas[i + 1] - sigmas[i], sigmas[i + 1], count, (hipStream_t)stream);
}

// The FluxPipeline.__call__ loop: for i: v = transformer(x, t_i); x = bf16(float(x) + (sigma_{i+1}-sigma_i) float(v)).
// latents [S_img, out_channels] bf16, updated in place; sigmas: n+1 host floats.  blend: FluxInpaintPipeline's step instead.
int denoise_loop(td_flux* f, void* latents, const float* sigmas, int n, const InpaintBlend* blend, void* stream) {
  block_cache_reset(f);      // (diffusers resets its cache state per pipeline call)
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
  for (int k = 0; k < count; ++k) { fs[k]->attn_variant = count > 1 ? multi_variant : 0; fs[k]->shared_chip = count > 1; block_cache_reset(fs[k]); }
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
  TD_CHECK_ARG(pos->S_img == neg->S_img && pos->m->Cout == neg->m->Cout, "td_flux_denoise_cfg: the contexts disagree on the latents: S_img %d / %d, out_channels %d / %d",
               pos->S_img, neg->S_img, pos->m->Cout, neg->m->Cout);
  TD_CHECK_ARG(pos->S_ref == neg->S_ref, "td_flux_denoise_cfg: the contexts hold %d / %d reference tokens (set the image's reference tokens on both, or on neither)",
               pos->S_ref, neg->S_ref);
  TD_CHECK_ARG(pos->n_steps == neg->n_steps, "td_flux_denoise_cfg: the contexts are prepared for %d / %d timesteps", pos->n_steps, neg->n_steps);
  TD_CHECK_ARG(n > 0 && n <= pos->n_steps, "td_flux_denoise_cfg: n=%d exceeds the %d prepared timesteps", n, pos->n_steps);
  const long long count = (long long)pos->S_img * pos->m->Cout;
  TD_CHECK_ARG(!overlaps(latents, (size_t)count * 2, pos->vout, (size_t)count * 2) && !overlaps(latents, (size_t)count * 2, neg->vout, (size_t)count * 2),
               "td_flux_denoise_cfg: latents overlap a context's velocity buffer");
  block_cache_reset(pos);      // two contexts, two cache states: diffusers' separate cond / uncond cache contexts
  block_cache_reset(neg);
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
