// FLUX engine, the shared model (FluxModel, csrc/flux_model.h): the fused bf16 weight arena and its diffusers-named parameter table, the
// numeric configuration (precision, Linear classes, activation scales, attention mode), the 8-bit weight arena, int8 smoothing, the attention
// score bounds and the LoRA registry.  Nothing here touches a context's workspace; csrc/flux_engine.hip holds what runs on one.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "flux_model.h"

namespace {

struct ArenaPlan {
  int64_t off = 0;
  std::vector<std::pair<bf16_t**, int64_t>> fix;  // pointer-to-fill, offset
  void take(bf16_t** p, int64_t n) {
    fix.emplace_back(p, off);
    off += (n + 127) & ~int64_t(127);  // 256-byte aligned tensors
  }
  void take(FluxLinear& l) { take(&l.w, (int64_t)l.N * l.K); take(&l.b, l.N); }
};

void add_slot(FluxModel* m, const std::string& name, bf16_t* ptr, int64_t count) {
  m->index[name] = (int)m->slots.size();
  m->slots.push_back({name, ptr, count, count, 1});
}

// registers "<name>.weight" / "<name>.bias" of a Linear living at rows [row0, row0+out) of a fused matrix
void add_linear(FluxModel* m, const std::string& name, const FluxLinear& l, int64_t row0, int64_t out) {
  add_slot(m, name + ".weight", l.w + row0 * l.K, out * l.K);
  m->slots.back().rows = out; m->slots.back().cols = l.K;
  add_slot(m, name + ".bias", l.b + row0, out);
}

}  // namespace

int flux_model_create(const TdFluxConfig* cfg, int controlnet, int num_mode, int max_img_tokens, int max_txt_tokens, int max_steps, FluxModel** out) {
  const char* const fn = controlnet ? "td_flux_controlnet_create" : "td_flux_create";
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
  TD_CHECK_ARG(cfg->num_layers >= (controlnet ? 1 : 0) && cfg->num_single_layers >= 0, "%s: num_layers=%d, num_single_layers=%d", fn, cfg->num_layers, cfg->num_single_layers);
  if (controlnet) {
    TD_CHECK_ARG(c_out == cfg->in_channels, "td_flux_controlnet_create: in_channels=%d, out_channels=%d: a ControlNet reads the latents alone (its condition enters "
                 "through controlnet_x_embedder, not through the channel axis)", cfg->in_channels, c_out);
    TD_CHECK_ARG(num_mode >= 0 && num_mode <= 65536, "td_flux_controlnet_create: num_mode=%d", num_mode);
  }
  FluxModel* m = new FluxModel();
  m->cfg = *cfg;
  m->controlnet = controlnet != 0;
  m->num_mode = controlnet ? num_mode : 0;
  m->cfg.out_channels = c_out;
  m->Cin = cfg->in_channels; m->Cout = c_out; m->Ccond = cfg->in_channels - c_out;
  const int D = m->D = cfg->num_heads * cfg->head_dim;
  const int M = m->M = cfg->mlp_ratio * D;
  const int L = cfg->num_layers, Ls = cfg->num_single_layers;
  m->NMOD = L * 12 * D + Ls * 3 * D + (controlnet ? 0 : 2 * D);      // (a ControlNet has no norm_out)
  m->max_img = max_img_tokens; m->max_txt = max_txt_tokens; m->max_steps = max_steps;
  m->dbl.resize(L);
  m->sgl.resize(Ls);

  // ---- every Linear's shape; the block Linears' class, smoothing slot and replication table ------------
  auto shape = [](FluxLinear& l, int N, int K) { l.N = N; l.K = K; };
  shape(m->x_emb, D, m->Cin); shape(m->ctx_emb, D, cfg->joint_dim);
  shape(m->t1, D, 256); shape(m->t2, D, D); shape(m->g1, D, 256); shape(m->g2, D, D);
  shape(m->p1, D, cfg->pooled_dim); shape(m->p2, D, D);
  shape(m->mod, m->NMOD, D); shape(m->proj, m->Cout, D);
  if (controlnet) {      // its own Linears: plain shapes, cls = 0 (always bf16), outside m->linears (never quantised, never smoothed)
    shape(m->cn_x_emb, D, m->Cin);
    m->cn_dbl.resize(L); m->cn_sgl.resize(Ls);
    for (FluxLinear& l : m->cn_dbl) shape(l, D, D);
    for (FluxLinear& l : m->cn_sgl) shape(l, D, D);
  }
  // smoothed: its input channels take the next K slots of the smoothing vectors; ln_fed: it reads a LayerNorm output and takes the next replication table
  auto block_linear = [&](FluxLinear& l, int N, int K, unsigned cls, bool smoothed, bool ln_fed, int sm_fixed = 0) {
    shape(l, N, K);
    l.cls = cls;
    if (smoothed) { l.sm = m->smooth_n; l.sm_fixed = sm_fixed; m->smooth_n += K; }
    if (ln_fed) l.ext = m->n_ext++;
    m->linears.push_back(&l);
  };
  struct Kind { int N, K; unsigned cls; bool smoothed, ln_fed; };
  const Kind dbl_kinds[DOUBLE_LINEARS / 2] = {{3 * D, D, TD_FP8_QKV, true, true}, {D, D, TD_FP8_OUT, false, false},      // qkv, out
                                              {M, D, TD_FP8_FF1, true, true}, {D, M, TD_FP8_FF2, true, false}};          // ff1, ff2
  for (DoubleBlock& b : m->dbl)
    for (int k = 0; k < DOUBLE_LINEARS; ++k) {      // (the image and the text Linear of a kind sit side by side)
      const Kind& q = dbl_kinds[k / 2];
      block_linear(b.lin[k], q.N, q.K, q.cls, q.smoothed, q.ln_fed);
    }
  for (SingleBlock& b : m->sgl) {
    block_linear(b.lin[SINGLE_IN], 3 * D + M, D, TD_FP8_SINGLE_IN, true, true);
    block_linear(b.lin[SINGLE_OUT], D, D + M, TD_FP8_SINGLE_OUT, true, false, D);
  }

  // ---- weight arena (this order fixes every parameter's offset: checkpoints of td_flux_init_random depend on it) -----------
  ArenaPlan ap;
  for (FluxLinear* l : {&m->x_emb, &m->ctx_emb, &m->t1, &m->t2, &m->g1, &m->g2, &m->p1, &m->p2, &m->mod, &m->proj}) ap.take(*l);
  for (DoubleBlock& b : m->dbl) {
    for (int k : {QKV_IMG, QKV_CTX, OUT_IMG, OUT_CTX, FF1_IMG, FF2_IMG, FF1_CTX, FF2_CTX}) ap.take(b.lin[k]);      // (the image MLP ahead of the text MLP)
    ap.take(&b.norm_q, 128); ap.take(&b.norm_k, 128); ap.take(&b.norm_added_q, 128); ap.take(&b.norm_added_k, 128);
  }
  for (SingleBlock& b : m->sgl) {
    ap.take(b.lin[SINGLE_IN]); ap.take(b.lin[SINGLE_OUT]);
    ap.take(&b.norm_q, 128); ap.take(&b.norm_k, 128);
  }
  if (controlnet) {      // behind everything the transformer has: the shared part keeps the transformer's offsets
    ap.take(m->cn_x_emb);
    for (FluxLinear& l : m->cn_dbl) ap.take(l);
    for (FluxLinear& l : m->cn_sgl) ap.take(l);
    if (m->num_mode > 0) ap.take(&m->cn_mode, (int64_t)m->num_mode * D);
  }
  m->arena_elems = ap.off;
  hipError_t e = hipMalloc((void**)&m->arena, (size_t)ap.off * sizeof(bf16_t));
  if (e != hipSuccess) {
    td_set_error("%s: hipMalloc of %.2f GiB weight arena failed: %s", fn, ap.off * 2.0 / (1 << 30), hipGetErrorString(e));
    delete m;
    return TD_ERR_HIP;
  }
  for (auto& fx : ap.fix) *fx.first = m->arena + fx.second;

  // ---- parameter table under the diffusers state-dict names ----------------------------------------
  add_linear(m, "x_embedder", m->x_emb, 0, D);
  add_linear(m, "context_embedder", m->ctx_emb, 0, D);
  add_linear(m, "time_text_embed.timestep_embedder.linear_1", m->t1, 0, D);
  add_linear(m, "time_text_embed.timestep_embedder.linear_2", m->t2, 0, D);
  if (cfg->guidance_embeds) {
    add_linear(m, "time_text_embed.guidance_embedder.linear_1", m->g1, 0, D);
    add_linear(m, "time_text_embed.guidance_embedder.linear_2", m->g2, 0, D);
  }
  add_linear(m, "time_text_embed.text_embedder.linear_1", m->p1, 0, D);
  add_linear(m, "time_text_embed.text_embedder.linear_2", m->p2, 0, D);
  for (int i = 0; i < L; ++i) {
    const std::string p = "transformer_blocks." + std::to_string(i) + ".";
    const DoubleBlock& b = m->dbl[i];
    add_linear(m, p + "norm1.linear", m->mod, (int64_t)i * 12 * D, 6 * D);
    add_linear(m, p + "norm1_context.linear", m->mod, (int64_t)i * 12 * D + 6 * D, 6 * D);
    add_linear(m, p + "attn.to_q", b.lin[QKV_IMG], 0, D);
    add_linear(m, p + "attn.to_k", b.lin[QKV_IMG], D, D);
    add_linear(m, p + "attn.to_v", b.lin[QKV_IMG], 2 * D, D);
    add_linear(m, p + "attn.add_q_proj", b.lin[QKV_CTX], 0, D);
    add_linear(m, p + "attn.add_k_proj", b.lin[QKV_CTX], D, D);
    add_linear(m, p + "attn.add_v_proj", b.lin[QKV_CTX], 2 * D, D);
    add_linear(m, p + "attn.to_out.0", b.lin[OUT_IMG], 0, D);
    add_linear(m, p + "attn.to_add_out", b.lin[OUT_CTX], 0, D);
    add_slot(m, p + "attn.norm_q.weight", b.norm_q, 128);
    add_slot(m, p + "attn.norm_k.weight", b.norm_k, 128);
    add_slot(m, p + "attn.norm_added_q.weight", b.norm_added_q, 128);
    add_slot(m, p + "attn.norm_added_k.weight", b.norm_added_k, 128);
    add_linear(m, p + "ff.net.0.proj", b.lin[FF1_IMG], 0, M);
    add_linear(m, p + "ff.net.2", b.lin[FF2_IMG], 0, D);
    add_linear(m, p + "ff_context.net.0.proj", b.lin[FF1_CTX], 0, M);
    add_linear(m, p + "ff_context.net.2", b.lin[FF2_CTX], 0, D);
  }
  for (int i = 0; i < Ls; ++i) {
    const std::string p = "single_transformer_blocks." + std::to_string(i) + ".";
    const SingleBlock& b = m->sgl[i];
    add_linear(m, p + "norm.linear", m->mod, (int64_t)L * 12 * D + (int64_t)i * 3 * D, 3 * D);
    add_linear(m, p + "attn.to_q", b.lin[SINGLE_IN], 0, D);
    add_linear(m, p + "attn.to_k", b.lin[SINGLE_IN], D, D);
    add_linear(m, p + "attn.to_v", b.lin[SINGLE_IN], 2 * D, D);
    add_linear(m, p + "proj_mlp", b.lin[SINGLE_IN], 3 * D, M);
    add_linear(m, p + "proj_out", b.lin[SINGLE_OUT], 0, D);
    add_slot(m, p + "attn.norm_q.weight", b.norm_q, 128);
    add_slot(m, p + "attn.norm_k.weight", b.norm_k, 128);
  }
  if (!controlnet) {
    add_linear(m, "norm_out.linear", m->mod, (int64_t)L * 12 * D + (int64_t)Ls * 3 * D, 2 * D);
    add_linear(m, "proj_out", m->proj, 0, m->Cout);
  } else {
    add_linear(m, "controlnet_x_embedder", m->cn_x_emb, 0, D);
    for (int i = 0; i < L; ++i) add_linear(m, "controlnet_blocks." + std::to_string(i), m->cn_dbl[i], 0, D);
    for (int i = 0; i < Ls; ++i) add_linear(m, "controlnet_single_blocks." + std::to_string(i), m->cn_sgl[i], 0, D);
    if (m->num_mode > 0) {
      add_slot(m, "controlnet_mode_embedder.weight", m->cn_mode, (int64_t)m->num_mode * D);
      m->slots.back().rows = m->num_mode; m->slots.back().cols = D;
    }
  }
  *out = m;
  return TD_OK;
}

void flux_model_destroy(FluxModel* m) {
  if (m->lora) {
    for (auto& a : m->lora->adapters) for (auto& p : a.pairs) (void)hipFree(p.packed);
    for (auto& b : m->lora->base) (void)hipFree(b.second);
    delete m->lora;
  }
  for (IpAdapter& a : m->ip) if (a.w) (void)hipFree(a.w);
  (void)hipFree(m->arena);
  if (m->arena8) (void)hipFree(m->arena8);
  if (m->sm_ax) (void)hipFree(m->sm_ax);      // one allocation: ax | aw | s | inv | inv16
  if (m->sm_ext) (void)hipFree(m->sm_ext);
  delete m;
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
int flux_refresh_score_bounds(FluxModel* m) {
  TD_CHECK_HIP(hipDeviceSynchronize());      // weight loads ran on the callers' streams
  const float c = 0.08838834764831845f * 1.4426950408889634f * 128.0f * 1.02f;      // premul x head_dim, 2 % for the bf16 roundings of q' and k
  constexpr float LIMIT = 48.0f;
  m->dbl_bound.assign(m->dbl.size(), 0.f);
  m->sgl_bound.assign(m->sgl.size(), 0.f);
  for (size_t i = 0; i < m->dbl.size(); ++i) {
    float a, b, cq, ck;
    TD_TRY(norm_weight_max(m->dbl[i].norm_q, &a)); TD_TRY(norm_weight_max(m->dbl[i].norm_added_q, &cq));
    TD_TRY(norm_weight_max(m->dbl[i].norm_k, &b)); TD_TRY(norm_weight_max(m->dbl[i].norm_added_k, &ck));
    const float bound = c * fmaxf(a, cq) * fmaxf(b, ck);
    m->dbl_bound[i] = bound > 0.f && bound <= LIMIT ? bound : 0.f;
  }
  for (size_t i = 0; i < m->sgl.size(); ++i) {
    float a, b;
    TD_TRY(norm_weight_max(m->sgl[i].norm_q, &a)); TD_TRY(norm_weight_max(m->sgl[i].norm_k, &b));
    const float bound = c * a * b;
    m->sgl_bound[i] = bound > 0.f && bound <= LIMIT ? bound : 0.f;
  }
  m->bounds_dirty = false;
  return TD_OK;
}

namespace {

// 8-bit modes: quantise every block Linear (per output channel, OCP e4m3 or symmetric int8) from the bf16 arena as it stands NOW -- call
// after the checkpoint is loaded, and again after reloading parameters.  Embedders, modulation and the final
// projection stay bf16 (< 0.1 % of the FLOPs; the modulation GEMM runs once per image).
int set_precision(FluxModel* m, int precision, hipStream_t s) {
  ++m->hist_epoch;
  m->smooth_ready = false;      // the weights are quantised afresh below, unsmoothed: the next int8 forward calibrates again
  if (precision == TD_PRECISION_BF16) { m->precision = precision; return TD_OK; }
  TD_CHECK_ARG(m->D % 128 == 0 && m->M % 128 == 0, "td_flux_set_precision: fp8 needs inner widths that are multiples of 128");
  if (!m->arena8) {
    auto al = [](int64_t b) { return (b + 255) & ~int64_t(255); };
    // rows of the LayerNorm-fed Linears: room for the replicated input channels of the smoothed form
    auto row_bytes = [](const FluxLinear& l) { return (int64_t)l.K + (l.ext >= 0 ? SM_EXT : 0); };
    int64_t total = 0;
    for (const FluxLinear* l : m->linears) total += al(l->N * row_bytes(*l)) + al((int64_t)l->N * 4);
    hipError_t e = hipMalloc((void**)&m->arena8, (size_t)total);
    if (e != hipSuccess) {
      td_set_error("td_flux_set_precision: hipMalloc of %.2f GiB fp8 arena failed: %s", total / double(1 << 30), hipGetErrorString(e));
      return TD_ERR_HIP;
    }
    int64_t o = 0;
    for (FluxLinear* l : m->linears) {
      l->w8.q = (uint8_t*)(m->arena8 + o); o += al(l->N * row_bytes(*l));
      l->w8.s = (float*)(m->arena8 + o); o += al((int64_t)l->N * 4);
    }
  }
  for (const FluxLinear* l : m->linears)
    TD_TRY(td_quant_rows_fp8_launch(l->w, l->K, l->w8.q, l->K, l->w8.s, l->N, l->K, s, precision == TD_PRECISION_INT8));
  m->precision = precision;
  return TD_OK;
}

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

}  // namespace

// End of the calibration forward (stream s): the weights' input-channel maxima, the plan of every smoothed Linear (host), the int8 weights again.
int flux_finish_smoothing(FluxModel* m, hipStream_t s) {
  const int64_t n = m->smooth_n;
  TD_CHECK_HIP(hipMemsetAsync(m->sm_aw, 0, (size_t)n * 4, s));
  for (const FluxLinear* l : m->linears)
    if (l->sm >= 0) TD_TRY(td_col_amax_launch(l->w, l->K, l->N, l->K, m->sm_aw + l->sm, s));
  std::vector<float> ax(n), aw(n), sw(n), inv(n);
  std::vector<bf16_t> inv16(n);
  std::vector<int> ext((size_t)m->n_ext * SM_EXT, -1);
  TD_CHECK_HIP(hipMemcpyAsync(ax.data(), m->sm_ax, (size_t)n * 4, hipMemcpyDeviceToHost, s));      // (float bits of non-negative values)
  TD_CHECK_HIP(hipMemcpyAsync(aw.data(), m->sm_aw, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  TD_CHECK_HIP(hipStreamSynchronize(s));
  for (const FluxLinear* l : m->linears) {
    if (l->sm < 0) continue;
    for (int64_t c = l->sm; c < l->sm + l->sm_fixed; ++c) { sw[c] = 1.f; inv[c] = 1.f; }
    const int64_t o = l->sm + l->sm_fixed;
    smooth_plan(&ax[o], &aw[o], l->K - l->sm_fixed, &sw[o], &inv[o], l->ext >= 0 ? &ext[(size_t)l->ext * SM_EXT] : nullptr);
  }
  for (int64_t c = 0; c < n; ++c) {      // bf16 of a power of two: its top 16 bits
    unsigned u; std::memcpy(&u, &inv[c], 4);
    inv16[c] = (bf16_t)(u >> 16);
  }
  TD_CHECK_HIP(hipMemcpyAsync(m->sm_s, sw.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(m->sm_inv, inv.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(m->sm_inv16, inv16.data(), (size_t)n * 2, hipMemcpyHostToDevice, s));
  TD_CHECK_HIP(hipMemcpyAsync(m->sm_ext, ext.data(), ext.size() * sizeof(int), hipMemcpyHostToDevice, s));
  TD_CHECK_HIP(hipStreamSynchronize(s));      // the host vectors go out of scope below
  // int8 weights again: column factors, and for the LayerNorm-fed ones rows of K + SM_EXT bytes with the replicated channels behind the real ones
  for (const FluxLinear* l : m->linears) {
    if (l->sm < 0) continue;
    const int ld = l->ext >= 0 ? l->K + SM_EXT : l->K;
    TD_TRY(td_quant_rows_fp8_launch(l->w, l->K, l->w8.q, ld, l->w8.s, l->N, l->K, s, 1, nullptr, m->sm_s + l->sm));
    if (l->ext >= 0) TD_TRY(td_ext_cols_launch(l->w8.q, ld, l->N, l->K, m->sm_ext + (size_t)l->ext * SM_EXT, SM_EXT, s));
  }
  TD_CHECK_HIP(hipStreamSynchronize(s));      // other contexts' streams read these weights next
  m->smooth_ready = true;
  ++m->hist_epoch;                             // scales recorded under the unsmoothed form say nothing about the smoothed one
  return TD_OK;
}

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
int lora_remerge(FluxModel* m, const std::vector<int>& slots, hipStream_t s) {
  LoraState* ls = m->lora;
  for (int slot : slots)
    TD_CHECK_ARG(lora_active_on(ls, slot, nullptr, nullptr, nullptr), "td_flux_lora: more than %d active adapters on '%s'", TD_LORA_MAX_ADAPTERS,
                 m->slots[slot].name.c_str());
  auto touched = [&](int slot) {
    for (const LoraAdapter& a : ls->adapters) for (const LoraPair& p : a.pairs) if (p.slot == slot) return true;
    return false;
  };
  bool orphans = false;
  for (int slot : slots) {
    auto it = ls->base.find(slot);
    if (it == ls->base.end()) continue;
    const Slot& sl = m->slots[slot];
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
  ++m->weight_epoch;
  ++m->hist_epoch;
  m->smooth_ready = false;
  if (m->precision != TD_PRECISION_BF16) TD_TRY(set_precision(m, m->precision, s));      // the 8-bit weights again, from the merged ones
  return TD_OK;
}

std::vector<int> lora_all_slots(const LoraState* ls) {
  std::vector<int> v;
  for (const auto& b : ls->base) v.push_back(b.first);
  std::sort(v.begin(), v.end());
  return v;
}

// a parameter is about to be overwritten: bounds, history and the smoothing calibration are stale
void weights_changed(FluxModel* m) {
  m->bounds_dirty = true;
  ++m->hist_epoch;
  m->smooth_ready = false;
}

}  // namespace

// ---- synthetic checkpoint: counter-based N(0, std) (full-shape random init for throughput runs) ------
// Grid-stride: a launch carries at most 2^32 - 1 work-items (the dispatch packet's grid size is 32 bits and a larger product is
// truncated WITHOUT an error) -- the 11.9 B-parameter FLUX arena needs 5.95 G pairs.  The one-thread-per-pair form filled only
// the first 3.3 G elements of it (embedders + modulation matrix) and left every block weight at the allocator's zeros.
__global__ void td_fill_normal_kernel(bf16_t* dst, long long n, unsigned long long seed, float std, float mean, long long pair0) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long pair = (long long)blockIdx.x * blockDim.x + threadIdx.x; 2 * pair < n; pair += stride) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(pair0 + pair + 1);      // (pair0: dst is a piece of a larger fill)
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

int td_fill_normal_from_launch(bf16_t* dst, long long n, unsigned long long seed, float std, float mean, long long pair0, hipStream_t stream) {
  TD_CHECK_ARG(dst && n > 0 && pair0 >= 0, "td_fill_normal_bf16: empty buffer");
  const long long pairs = (n + 1) / 2;
  const long long blocks = (pairs + 255) / 256;
  hipLaunchKernelGGL(td_fill_normal_kernel, dim3((unsigned)(blocks < (1ll << 20) ? blocks : (1ll << 20))), dim3(256), 0, stream, dst, n, seed, std, mean, pair0);
  TD_CHECK_LAUNCH();
  return TD_OK;
}

extern "C" {

int64_t td_flux_param_elems(const td_flux* f) { return f ? f->m->arena_elems : 0; }
int td_flux_num_params(const td_flux* f) { return f ? (int)f->m->slots.size() : 0; }

int td_flux_param_info(const td_flux* f, int idx, char* name_buf, int buf_len, int64_t* count) {
  TD_CHECK_ARG(f && idx >= 0 && idx < (int)f->m->slots.size(), "td_flux_param_info: index %d out of range", idx);
  const Slot& s = f->m->slots[idx];
  if (name_buf && buf_len > 0) {
    strncpy(name_buf, s.name.c_str(), buf_len - 1);
    name_buf[buf_len - 1] = 0;
  }
  if (count) *count = s.count;
  return TD_OK;
}

int td_flux_load_param(td_flux* f, const char* name, const void* src, int64_t count, void* stream) {
  TD_CHECK_ARG(f && name && src, "td_flux_load_param: null argument");
  FluxModel* m = f->m;
  weights_changed(m);
  auto it = m->index.find(name);
  TD_CHECK_ARG(it != m->index.end(), "td_flux_load_param: unknown parameter '%s'", name);
  const Slot& s = m->slots[it->second];
  TD_CHECK_ARG(s.count == count, "td_flux_load_param: '%s' expects %lld elements, got %lld", name, (long long)s.count, (long long)count);
  TD_CHECK_ARG(!m->lora || !m->lora->base.count(it->second), "td_flux_load_param: '%s' carries LoRA adapters (its base copy would go stale): clear the adapters first "
               "(td_flux_lora_clear)", name);
  TD_CHECK_HIP(hipMemcpyAsync(s.ptr, src, (size_t)count * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

int td_flux_read_param(td_flux* f, const char* name, void* dst, int64_t count, void* stream) {
  TD_CHECK_ARG(f && name && dst, "td_flux_read_param: null argument");
  auto it = f->m->index.find(name);
  TD_CHECK_ARG(it != f->m->index.end(), "td_flux_read_param: unknown parameter '%s'", name);
  const Slot& s = f->m->slots[it->second];
  TD_CHECK_ARG(s.count == count, "td_flux_read_param: '%s' holds %lld elements, the destination %lld", name, (long long)s.count, (long long)count);
  TD_CHECK_HIP(hipMemcpyAsync(dst, s.ptr, (size_t)count * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

int td_flux_param_shape(const td_flux* f, const char* name, int64_t* rows, int64_t* cols) {
  TD_CHECK_ARG(f && name, "td_flux_param_shape: null argument");
  auto it = f->m->index.find(name);
  TD_CHECK_ARG(it != f->m->index.end(), "td_flux_param_shape: unknown parameter '%s'", name);
  if (rows) *rows = f->m->slots[it->second].rows;
  if (cols) *cols = f->m->slots[it->second].cols;
  return TD_OK;
}

int td_fill_normal_bf16(void* dst, int64_t n, uint64_t seed, float std, float mean, void* stream) {
  return td_fill_normal_from_launch((bf16_t*)dst, (long long)n, (unsigned long long)seed, std, mean, 0, (hipStream_t)stream);
}

int td_flux_init_random(td_flux* f, uint64_t seed, float std, void* stream) {
  TD_CHECK_ARG(f, "td_flux_init_random: null handle");
  FluxModel* m = f->m;
  TD_CHECK_ARG(!m->lora || m->lora->base.empty(), "td_flux_init_random: %d parameters carry LoRA adapters (their base copies would go stale): clear the adapters first "
               "(td_flux_lora_clear)", m->lora ? (int)m->lora->base.size() : 0);
  weights_changed(m);
  TD_TRY(td_fill_normal_bf16(m->arena, m->arena_elems, seed, std, 0.f, stream));
  for (const Slot& s : m->slots)
    if (s.count == 128 && s.name.find(".norm_") != std::string::npos)
      TD_TRY(td_fill_normal_bf16(s.ptr, s.count, seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(s.ptr - m->arena + 1)), 0.1f, 1.0f, stream));
  return TD_OK;
}

// Which block Linears run on 8-bit operands in the 8-bit modes (TD_FP8_* class bits).
int td_flux_set_fp8_gemms(td_flux* f, unsigned mask) {
  TD_CHECK_ARG(f && f->root, "td_flux_set_fp8_gemms: set it on the parent context (forks follow it)");
  TD_CHECK_ARG((mask & ~(unsigned)TD_FP8_ALL_GEMMS) == 0, "td_flux_set_fp8_gemms: unknown bits in mask 0x%x", mask);
  f->m->fp8_mask = mask;
  ++f->m->hist_epoch;
  return TD_OK;
}

// TD_PRECISION_INT8 only: where the per-token activation scales of the attention-output / MLP operands come from.  0 (default): measured
// on the spot -- one quantisation pass per tensor.  1: from the maxima the PREVIOUS denoise step accumulated for the same tensor and
// token, times 1.25 (values beyond that clip at +-127): the MLP intermediate then leaves the producing GEMM epilogue as int8 and the
// passes over it disappear; the first step of an image, and any step that does not follow its predecessor, runs the mode-0 path.
int td_flux_set_act_scales(td_flux* f, int mode) {
  TD_CHECK_ARG(f && f->root && (mode == 0 || mode == 1), "td_flux_set_act_scales: parent context, mode 0 or 1");
  f->m->act_scale_mode = mode;
  ++f->m->hist_epoch;
  return TD_OK;
}

// TD_PRECISION_INT8 only: per-channel smoothing of the activations that carry outlier channels (SmoothQuant's balance, alpha = 1/2, factors rounded
// to powers of two).  Per-token symmetric int8 gives every channel of a row the step max|row| / 127: a trained DiT's few residual-stream /
// MLP channels that run tens of times above the rest then leave the rest 2-3 bits.  With mode 1 the FIRST int8 forward after the mode, the
// precision or a parameter changed runs on the bf16 path and records, per input channel of the Linears fed by a LayerNorm output (q|k|v, ff.net.0,
// proj_mlp) or by an MLP intermediate (ff.net.2, proj_out's MLP half), the largest activation; s = 2^rint(log2 sqrt(max|x_c| / max|W[:, c]|)) then
// divides that activation channel (inside the LayerNorm kernel, the producing GEMM's int8 epilogue or the quantisation pass) and multiplies the
// weight's input channel before the weight is quantised again.  Powers of two: x / s and W s are exact, the product is the unsmoothed one, only
// the quantisation steps move.  0 (default) = off.
int td_flux_set_smoothing(td_flux* f, int mode) {
  TD_CHECK_ARG(f && f->root && (mode == 0 || mode == 1), "td_flux_set_smoothing: parent context, mode 0 or 1");
  FluxModel* m = f->m;
  if (mode == 1 && !m->sm_ax) {
    const int64_t n = m->smooth_n;
    char* base = nullptr;
    TD_CHECK_HIP(hipMalloc((void**)&base, (size_t)n * (4 + 4 + 4 + 4 + 2)));
    m->sm_ax = (unsigned*)base; m->sm_aw = m->sm_ax + n; m->sm_s = (float*)(m->sm_aw + n); m->sm_inv = m->sm_s + n; m->sm_inv16 = (bf16_t*)(m->sm_inv + n);
    TD_CHECK_HIP(hipMalloc((void**)&m->sm_ext, (size_t)m->n_ext * SM_EXT * sizeof(int)));
  }
  if (mode != m->smooth_mode) {
    ++m->hist_epoch;
    m->smooth_ready = false;
    // leaving the mode: the int8 weights must lose their column factors -- quantise them again from the bf16 arena
    if (mode == 0 && m->smooth_mode == 1 && m->precision == TD_PRECISION_INT8 && m->arena8) { m->smooth_mode = 0; return set_precision(m, TD_PRECISION_INT8, nullptr); }
  }
  m->smooth_mode = mode;
  return TD_OK;
}

// The joint attention of every block: TD_ATTENTION_BF16 (default, the reference graph's arithmetic) or TD_ATTENTION_FP8 -- QK^T and P.V on
// the e4m3 matrix instruction (csrc/attention_fp8.hip).  Independent of td_flux_set_precision; meant for the 8-bit modes, where the
// attention is otherwise a quarter of the image.
int td_flux_set_attention(td_flux* f, int mode) {
  TD_CHECK_ARG(f && f->root && (mode == TD_ATTENTION_BF16 || mode == TD_ATTENTION_FP8), "td_flux_set_attention: parent context, TD_ATTENTION_BF16 or TD_ATTENTION_FP8");
  TD_CHECK_ARG(!f->m->controlnet || mode == TD_ATTENTION_BF16, "td_flux_set_attention: mode %d on a ControlNet model: the side network runs in bf16 only", mode);
  f->m->attn_mode = mode;
  ++f->m->hist_epoch;
  return TD_OK;
}

int td_flux_set_precision(td_flux* f, int precision, void* stream) {
  TD_CHECK_ARG(f && (precision == TD_PRECISION_BF16 || precision == TD_PRECISION_FP8_E4M3 || precision == TD_PRECISION_INT8), "td_flux_set_precision: unknown precision %d", precision);
  TD_CHECK_ARG(f->root, "td_flux_set_precision: set the precision on the parent context (forks follow it)");
  TD_CHECK_ARG(!f->m->controlnet || precision == TD_PRECISION_BF16, "td_flux_set_precision: precision %d on a ControlNet model: the side network runs in bf16 only "
               "(the main transformer may be in any mode)", precision);
  return set_precision(f->m, precision, (hipStream_t)stream);
}

int td_flux_lora_load(td_flux* f, const char* adapter, const char* param, const void* A, const void* B, int rank, float scale, void* stream) {
  TD_CHECK_ARG(f && adapter && param && A && B, "td_flux_lora_load: null argument");
  TD_CHECK_ARG(f->root, "td_flux_lora_load: '%s': adapters belong to the parent context (forks see its weights)", param);
  TD_CHECK_ARG(adapter[0], "td_flux_lora_load: empty adapter name");
  TD_CHECK_ARG(!f->m->controlnet, "td_flux_lora_load: '%s' on a ControlNet model: adapters on the side network are not built (the main transformer takes them)", param);
  FluxModel* m = f->m;
  auto it = m->index.find(param);
  TD_CHECK_ARG(it != m->index.end(), "td_flux_lora_load: unknown parameter '%s'", param);
  const int slot = it->second;
  const Slot& sl = m->slots[slot];
  const size_t pl = strlen(param);
  TD_CHECK_ARG(sl.cols > 1 && pl > 7 && strcmp(param + pl - 7, ".weight") == 0, "td_flux_lora_load: '%s' is not the weight of a Linear (%lld elements, 1-D): "
               "bias and norm-scale deltas are not built", param, (long long)sl.count);
  TD_CHECK_ARG(rank >= 1, "td_flux_lora_load: '%s': rank=%d must be at least 1", param, rank);
  TD_CHECK_ARG(std::isfinite(scale), "td_flux_lora_load: '%s': scale is not finite", param);
  TD_CHECK_ARG((uintptr_t)A % 16 == 0 && (uintptr_t)B % 16 == 0, "td_flux_lora_load: '%s': A and B must be 16-byte aligned", param);
  TD_CHECK_ARG(sl.cols % 64 == 0 && sl.rows % 8 == 0 && sl.rows < (1ll << 31) && sl.cols < (1ll << 31), "td_flux_lora_load: '%s' is [%lld, %lld]: the merge "
               "needs rows %% 8 == 0 and columns %% 64 == 0", param, (long long)sl.rows, (long long)sl.cols);
  if (!m->lora) m->lora = new LoraState();
  LoraState* ls = m->lora;
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
  TD_CHECK_ARG(f->root, "td_flux_lora_set_adapters: adapters belong to the parent context (forks see its weights)");
  LoraState* ls = f->m->lora;
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
      td_set_error("td_flux_lora_set_adapters: more than %d active adapters on '%s'", TD_LORA_MAX_ADAPTERS, f->m->slots[slot].name.c_str());
      return TD_ERR_INVALID;
    }
  return lora_remerge(f->m, slots, (hipStream_t)stream);
}

int td_flux_lora_delete(td_flux* f, const char* adapter, void* stream) {
  TD_CHECK_ARG(f && adapter, "td_flux_lora_delete: null argument");
  TD_CHECK_ARG(f->root, "td_flux_lora_delete: adapters belong to the parent context (forks see its weights)");
  LoraState* ls = f->m->lora;
  const int ai = lora_find(ls, adapter);
  TD_CHECK_ARG(ai >= 0, "td_flux_lora_delete: unknown adapter '%s'", adapter);
  TD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));      // its operands may still be read by a merge in flight
  std::vector<int> slots;
  for (LoraPair& p : ls->adapters[ai].pairs) { slots.push_back(p.slot); (void)hipFree(p.packed); }
  ls->adapters.erase(ls->adapters.begin() + ai);
  return lora_remerge(f->m, slots, (hipStream_t)stream);
}

int td_flux_lora_clear(td_flux* f, void* stream) {
  TD_CHECK_ARG(f, "td_flux_lora_clear: null handle");
  TD_CHECK_ARG(f->root, "td_flux_lora_clear: adapters belong to the parent context (forks see its weights)");
  LoraState* ls = f->m->lora;
  if (!ls || (ls->adapters.empty() && ls->base.empty())) return TD_OK;
  TD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (LoraAdapter& a : ls->adapters) for (LoraPair& p : a.pairs) (void)hipFree(p.packed);
  ls->adapters.clear();
  return lora_remerge(f->m, lora_all_slots(ls), (hipStream_t)stream);
}

int td_flux_lora_info(const td_flux* f, int* n_adapters, int* n_params_touched, int64_t* bytes_held) {
  TD_CHECK_ARG(f, "td_flux_lora_info: null handle");
  const LoraState* ls = f->m->lora;
  int64_t bytes = 0;
  if (ls) {
    for (const LoraAdapter& a : ls->adapters) for (const LoraPair& p : a.pairs) bytes += p.bytes;
    for (const auto& b : ls->base) bytes += f->m->slots[b.first].count * 2;
  }
  if (n_adapters) *n_adapters = ls ? (int)ls->adapters.size() : 0;
  if (n_params_touched) *n_params_touched = ls ? (int)ls->base.size() : 0;
  if (bytes_held) *bytes_held = bytes;
  return TD_OK;
}

// ---- IP-Adapter slots (the model's half; td_flux_set_ip_image_embeds and the block loop's half are in csrc/flux_engine.hip) ------------------------
static int ip_slot_arg(const char* fn, const td_flux* f, int slot) {
  TD_CHECK_ARG(f, "%s: null handle", fn);
  TD_CHECK_ARG(f->root, "%s: adapters belong to the parent context (forks share its model)", fn);
  TD_CHECK_ARG(!f->m->controlnet, "%s: a ControlNet takes no IP-Adapter", fn);
  TD_CHECK_ARG(slot >= 0 && slot < TD_IP_MAX_ADAPTERS, "%s: slot %d outside 0 .. %d", fn, slot, TD_IP_MAX_ADAPTERS - 1);
  return TD_OK;
}

static void ip_free_slot(FluxModel* m, int slot) {
  IpAdapter& a = m->ip[slot];
  if (a.w) (void)hipFree(a.w);
  a = IpAdapter();
  a.epoch = ++m->ip_epoch;      // contexts that hold K / V of the old weights are stale
}

int td_flux_ip_adapter_add(td_flux* f, int num_tokens, int embed_dim, int* slot_out) {
  TD_TRY(ip_slot_arg("td_flux_ip_adapter_add", f, 0));
  TD_CHECK_ARG(slot_out, "td_flux_ip_adapter_add: null slot pointer");
  TD_CHECK_ARG(num_tokens >= 1 && num_tokens <= TD_IP_MAX_KEYS, "td_flux_ip_adapter_add: num_tokens=%d outside 1 .. %d (TD_IP_MAX_KEYS)", num_tokens, TD_IP_MAX_KEYS);
  TD_CHECK_ARG(embed_dim >= 8 && embed_dim % 8 == 0 && embed_dim <= 65536, "td_flux_ip_adapter_add: embed_dim=%d must be a multiple of 8 in 8 .. 65536", embed_dim);
  FluxModel* m = f->m;
  int slot = -1;
  for (int i = 0; i < TD_IP_MAX_ADAPTERS && slot < 0; ++i) if (!m->ip[i].used) slot = i;
  TD_CHECK_ARG(slot >= 0, "td_flux_ip_adapter_add: all %d slots are taken (td_flux_ip_adapter_remove frees one)", TD_IP_MAX_ADAPTERS);
  IpAdapter a;
  a.num_tokens = num_tokens; a.E = embed_dim; a.E_pad = (embed_dim + 63) & ~63;
  const int64_t J = m->cfg.joint_dim, D = m->D, L = m->cfg.num_layers, NJ = (int64_t)num_tokens * J;
  const int64_t total = NJ * a.E_pad + NJ + 2 * J + L * 2 * (D * J + D);
  hipError_t e = hipMalloc((void**)&a.w, (size_t)total * 2);
  if (e != hipSuccess) {
    td_set_error("td_flux_ip_adapter_add: hipMalloc of %.2f GiB of adapter weights failed: %s", total * 2 / double(1 << 30), hipGetErrorString(e));
    return TD_ERR_HIP;
  }
  TD_CHECK_HIP(hipMemset(a.w, 0, (size_t)total * 2));      // (the padding columns of proj.weight stay zero)
  bf16_t* p = a.w;
  auto put = [&](const std::string& name, int64_t rows, int64_t cols, int64_t ld) {
    a.params[name] = IpParam{p, rows * cols, (int)rows, (int)cols, (int)ld, false};
    p += rows * ld;
  };
  put("image_proj.proj.weight", NJ, a.E, a.E_pad);
  put("image_proj.proj.bias", 1, NJ, NJ);
  put("image_proj.norm.weight", 1, J, J);
  put("image_proj.norm.bias", 1, J, J);
  for (int i = 0; i < L; ++i)
    for (const char* kv : {"to_k_ip", "to_v_ip"}) {
      const std::string base = "ip_adapter." + std::to_string(i) + "." + kv;
      put(base + ".weight", D, J, J);
      put(base + ".bias", 1, D, D);
    }
  a.scale.assign((size_t)L, 1.0f);
  a.used = true;
  a.epoch = ++m->ip_epoch;
  m->ip[slot] = std::move(a);
  *slot_out = slot;
  return TD_OK;
}

int td_flux_ip_adapter_load_param(td_flux* f, int slot, const char* name, const void* data, int64_t count, void* stream) {
  TD_TRY(ip_slot_arg("td_flux_ip_adapter_load_param", f, slot));
  TD_CHECK_ARG(name && data, "td_flux_ip_adapter_load_param: null argument");
  IpAdapter& a = f->m->ip[slot];
  TD_CHECK_ARG(a.used, "td_flux_ip_adapter_load_param: '%s': slot %d holds no adapter (td_flux_ip_adapter_add)", name, slot);
  auto it = a.params.find(name);
  TD_CHECK_ARG(it != a.params.end(), "td_flux_ip_adapter_load_param: unknown parameter '%s' (slot %d: %d tokens, %d double blocks)", name, slot, a.num_tokens,
               f->m->cfg.num_layers);
  IpParam& q = it->second;
  TD_CHECK_ARG(q.count == count, "td_flux_ip_adapter_load_param: '%s' expects %lld elements ([%d, %d]), got %lld", name, (long long)q.count, q.rows, q.cols, (long long)count);
  TD_CHECK_HIP(hipMemcpy2DAsync(q.ptr, (size_t)q.ld * 2, data, (size_t)q.cols * 2, (size_t)q.cols * 2, (size_t)q.rows, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  q.loaded = true;
  a.epoch = ++f->m->ip_epoch;
  return TD_OK;
}

int td_flux_ip_adapter_remove(td_flux* f, int slot) {
  TD_TRY(ip_slot_arg("td_flux_ip_adapter_remove", f, slot < 0 ? 0 : slot));
  TD_CHECK_ARG(slot >= -1, "td_flux_ip_adapter_remove: slot %d (-1 removes all)", slot);
  TD_CHECK_HIP(hipDeviceSynchronize());      // a context may still be computing K / V from these weights
  for (int i = 0; i < TD_IP_MAX_ADAPTERS; ++i)
    if ((slot < 0 || slot == i) && f->m->ip[i].used) ip_free_slot(f->m, i);
  return TD_OK;
}

int td_flux_set_ip_adapter_scale(td_flux* f, int slot, const float* per_block, int n) {
  TD_TRY(ip_slot_arg("td_flux_set_ip_adapter_scale", f, slot));
  IpAdapter& a = f->m->ip[slot];
  const int L = f->m->cfg.num_layers;
  TD_CHECK_ARG(a.used, "td_flux_set_ip_adapter_scale: slot %d holds no adapter", slot);
  TD_CHECK_ARG(per_block && (n == 1 || n == L), "td_flux_set_ip_adapter_scale: %d scales given; one for all blocks or one per double block (%d)", n, L);
  for (int i = 0; i < n; ++i) TD_CHECK_ARG(std::isfinite(per_block[i]), "td_flux_set_ip_adapter_scale: scale %d is not finite", i);
  for (int i = 0; i < L; ++i) a.scale[i] = per_block[n == 1 ? 0 : i];
  return TD_OK;
}

int td_flux_ip_adapter_info(const td_flux* f, int slot, int* used, int* num_tokens, int* embed_dim, int* embeds_set, int* n_keys) {
  TD_CHECK_ARG(f && slot >= 0 && slot < TD_IP_MAX_ADAPTERS, "td_flux_ip_adapter_info: null handle or slot %d outside 0 .. %d", slot, TD_IP_MAX_ADAPTERS - 1);
  const IpAdapter& a = f->m->ip[slot];
  if (used) *used = a.used;
  if (num_tokens) *num_tokens = a.num_tokens;
  if (embed_dim) *embed_dim = a.E;
  if (embeds_set) *embeds_set = f->ip[slot].set;
  if (n_keys) *n_keys = f->ip[slot].set ? f->ip[slot].n_keys : 0;
  return TD_OK;
}

}  // extern "C"
