// FLUX engine, internal structures: the shared model (FluxModel: weights, numeric configuration, LoRA registry -- csrc/flux_model.hip) and the
// per-image context (td_flux: workspace, conditioning, schedule, history, trace -- csrc/flux_engine.hip).  Every context holds a pointer to ONE
// model; the root context (td_flux_create) owns it and frees it, forks (td_flux_fork) borrow it and must not outlive the root.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "td_kernels.h"
#include "../../include/thinkdiff_hip.h"

struct Slot {
  std::string name;
  bf16_t* ptr;
  int64_t count;
  int64_t rows, cols;      // [N, K] of a Linear's weight; [count, 1] of a 1-D parameter
};

// LoRA adapters (td_flux_lora_*; root context).  An adapter is a set of low-rank pairs, each on one Linear weight slot, kept in the merge kernel's
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

// IP-Adapter (td_flux_ip_adapter_*; root context; [ext] diffusers FluxIPAdapterMixin, restated).  One slot = one adapter: the image projection
// (Linear E -> num_tokens x J, LayerNorm over J) and, per double block, to_k_ip / to_v_ip (Linear J -> D, bias).  All of it stays bf16 in every
// precision mode, in ONE allocation of its own (adapters come and go; the fused weight arena does not move).  proj.weight is held with its rows
// zero-padded to E_pad = a multiple of the GEMM's k-tile (the padding adds exact zeros).
struct IpParam {
  bf16_t* ptr;
  int64_t count;           // elements the caller supplies: rows x cols
  int rows, cols, ld;      // ld: row stride in the allocation (cols, or E_pad for proj.weight)
  bool loaded;
};
struct IpAdapter {
  bool used = false;
  int num_tokens = 0, E = 0, E_pad = 0;
  bf16_t* w = nullptr;
  std::unordered_map<std::string, IpParam> params;
  std::vector<float> scale;      // per double block (td_flux_set_ip_adapter_scale; default 1.0)
  // td_flux_ip_adapter_add / _load_param / _remove give the slot a new epoch (from FluxModel::ip_epoch); td_flux_set_ip_image_embeds records it on
  // its context -- the K / V it computed are values of these weights -- and a forward refuses a context whose record is older.
  int epoch = 0;
};

// 8-bit modes (td_flux_set_precision): e4m3 / int8 copy of a block weight [rows, K] + one dequantisation scale per output channel
struct Fp8Mat {
  uint8_t* q = nullptr;
  float* s = nullptr;
};
// int8 smoothing: the Linears fed by a LayerNorm output (q|k|v, ff.net.0, proj_mlp | q|k|v of the single blocks) may carry up to SM_EXT replicated
// input channels behind their K real ones (one more k-tile); their int8 weights and the quantised LayerNorm rows are allocated for K + SM_EXT
constexpr int SM_EXT = 128;

// One Linear.  The embedders, the modulation matrix and the final projection use w / b / N / K only (cls = 0: always bf16); a block Linear also
// carries what the 8-bit modes need.  Everything but w8 is fixed at creation (flux_model_create is the one place that writes shapes and offsets).
struct FluxLinear {
  bf16_t *w = nullptr, *b = nullptr;      // [N, K], [N] in the bf16 arena
  int N = 0, K = 0;
  unsigned cls = 0;        // its TD_FP8_* class bit (td_flux_set_fp8_gemms)
  Fp8Mat w8;               // rows of K bytes, or of K + SM_EXT in the smoothed form of a Linear with ext >= 0
  int64_t sm = -1;         // offset of its K input channels in the smoothing vectors (FluxModel::sm_*); -1: not smoothed (the out-projections)
  int sm_fixed = 0;        // its first sm_fixed input channels keep factor 1 (the attention half of a single block's proj_out operand)
  int ext = -1;            // its replicated-channel table is sm_ext + ext * SM_EXT; -1: no replication (the MLP-fed Linears, the out-projections)
};
// Block Linears in fixed positions.  The order is the one of the 8-bit arena, of the quantisation launches and -- the out-projections aside -- of
// the smoothing vectors.
enum { QKV_IMG, QKV_CTX, OUT_IMG, OUT_CTX, FF1_IMG, FF1_CTX, FF2_IMG, FF2_CTX, DOUBLE_LINEARS };
struct DoubleBlock {
  FluxLinear lin[DOUBLE_LINEARS];
  bf16_t *norm_q, *norm_k, *norm_added_q, *norm_added_k;
};
enum { SINGLE_IN, SINGLE_OUT, SINGLE_LINEARS };      // [3D + M, D] = to_q | to_k | to_v | proj_mlp; proj_out [D, D + M]
struct SingleBlock {
  FluxLinear lin[SINGLE_LINEARS];
  bf16_t *norm_q, *norm_k;
};

struct FluxModel {
  TdFluxConfig cfg;
  int D = 0, M = 0, NMOD = 0;
  int max_img = 0, max_txt = 0, max_steps = 0;      // capacities of every context
  // channel conditioning (FLUX.1 Fill / Canny / Depth): x_embedder reads Cin = Cout + Ccond columns, everything from proj_out on has Cout
  int Cin = 0, Cout = 0, Ccond = 0;
  // weights
  bf16_t* arena = nullptr;
  int64_t arena_elems = 0;
  std::vector<Slot> slots;
  std::unordered_map<std::string, int> index;
  FluxLinear x_emb, ctx_emb, t1, t2, g1, g2, p1, p2, mod, proj;
  // A ControlNet side network (td_flux_controlnet_create; [ext] diffusers FluxControlNetModel): the same embedders and blocks, no final norm and
  // no proj_out (NMOD without the final-norm share), and its own always-bf16 Linears -- controlnet_x_embedder [D, Cin], one output Linear [D, D]
  // behind every double / single block -- plus the mode embedding [num_mode, D] of the "union" checkpoints (num_mode == 0: none).
  bool controlnet = false;
  int num_mode = 0;
  FluxLinear cn_x_emb;
  std::vector<FluxLinear> cn_dbl, cn_sgl;
  bf16_t* cn_mode = nullptr;
  std::vector<DoubleBlock> dbl;
  std::vector<SingleBlock> sgl;
  std::vector<FluxLinear*> linears;      // every block Linear, in block order
  // Upper bounds of the attention scores of each block (bf16 attention: TdAttnParams::score_bound), from its QK-RMSNorm weights: the norm
  // leaves |q'|, |k| <= sqrt(128) x max|w|, so q'.k <= premul x 128 x max|w_q| x max|w_k|.  Refreshed lazily after weights change.
  std::vector<float> dbl_bound, sgl_bound;
  bool bounds_dirty = true;
  // numeric configuration
  int precision = TD_PRECISION_BF16;
  unsigned fp8_mask = TD_FP8_ALL_GEMMS;   // which block Linears run on the 8-bit path in the 8-bit modes (td_flux_set_fp8_gemms)
  int attn_mode = 0;                      // TD_ATTENTION_BF16 / TD_ATTENTION_FP8 (td_flux_set_attention)
  int act_scale_mode = 0;                 // int8: 0 = per-token scales measured on the spot (a pass per tensor), 1 = history (td_flux_set_act_scales)
  char* arena8 = nullptr;                 // the Fp8Mat of every block Linear
  // int8 smoothing (td_flux_set_smoothing).  Per input channel of the Linears that read a LayerNorm output or an MLP intermediate, a power-of-two
  // factor s: the activation channel is divided by s where it is quantised, the weight's input channel multiplied by s before ITS quantisation.
  // The factors come from ONE calibration forward (the first forward after the mode / the weights / the precision changed, run on the bf16 path
  // with per-channel maxima collected along the way).  Layout of every vector below, in channels (FluxLinear::sm): double block i at
  // i (4 D + 2 M): qkv_img[D] qkv_ctx[D] ff1_img[D] ff1_ctx[D] ff2_img[M] ff2_ctx[M]; single block i at L (4 D + 2 M) + i (2 D + M): w1[D]
  // w2[D + M] (the attention half of w2's operand is never smoothed: its maxima stay 0 and its factors 1).
  int smooth_mode = 0;
  bool smooth_ready = false;
  int n_ext = 0;                                    // Linears with a replicated-channel table: 4 L + Ls
  int* sm_ext = nullptr;                            // [n_ext][SM_EXT] source channel or -1
  int64_t smooth_n = 0;
  unsigned *sm_ax = nullptr, *sm_aw = nullptr;      // channel maxima of the activations / of the weights' input channels (float bits)
  float *sm_s = nullptr, *sm_inv = nullptr;         // s, 1 / s
  bf16_t* sm_inv16 = nullptr;                       // 1 / s as bf16 (the LayerNorm and GEMM epilogue kernels read it beside their bf16 operands)
  LoraState* lora = nullptr;
  IpAdapter ip[TD_IP_MAX_ADAPTERS];
  int ip_epoch = 0;
  // td_flux_lora_set_adapters / delete / clear bump the weight epoch; td_flux_set_condition / td_flux_set_timesteps record it on their context
  // (both precompute values from weights), and a forward refuses a context prepared under an older one.
  int weight_epoch = 0;
  // Every setter that changes weights, precision, Linear classes, scale mode or attention mode bumps the history epoch: a context trusts its
  // per-step history (td_flux::href, hs_*) only when it was recorded in the current one.
  int hist_epoch = 0;
  // First-block cache (td_flux_set_block_cache / _schedule; include/thinkdiff_hip.h spells the semantics): 0 off, 1 threshold, 2 fixed schedule.
  // The settings are the model's -- forks follow their parent -- and every change bumps bc_epoch, which voids every context's cache state.
  int bc_mode = 0;
  float bc_threshold = 0.f;
  std::vector<unsigned char> bc_schedule;
  int bc_epoch = 0;
};

// int8 smoothing: the first forward after a change calibrates -- it runs on the bf16 path and collects channel maxima
inline bool flux_calibrating(const FluxModel* m) { return m->precision == TD_PRECISION_INT8 && m->smooth_mode == 1 && !m->smooth_ready; }
inline bool flux_smoothed(const FluxModel* m) { return m->precision == TD_PRECISION_INT8 && m->smooth_mode == 1 && m->smooth_ready; }
// the Linear classes that run on 8-bit operands right now
inline unsigned flux_mask8(const FluxModel* m) { return (m->precision != TD_PRECISION_BF16 && !flux_calibrating(m)) ? m->fp8_mask : 0u; }
// contraction length (= row stride of w8.q) of a Linear's 8-bit form
inline int flux_k8(const FluxModel* m, const FluxLinear& l) { return l.K + (l.ext >= 0 && flux_smoothed(m) ? SM_EXT : 0); }

// csrc/flux_model.hip.  flux_model_create validates the configuration (td_flux_create's argument errors) and allocates arena + parameter table.
// controlnet: the side-network kind (num_mode: rows of its mode embedding, 0 = none); 0, 0: the transformer.
int flux_model_create(const TdFluxConfig* cfg, int controlnet, int num_mode, int max_img_tokens, int max_txt_tokens, int max_steps, FluxModel** out);
void flux_model_destroy(FluxModel* m);
int flux_refresh_score_bounds(FluxModel* m);
int flux_finish_smoothing(FluxModel* m, hipStream_t s);      // end of the calibration forward on stream s

struct td_flux {
  FluxModel* m = nullptr;
  bool root = false;                        // created by td_flux_create: owns the model; the setters of model state accept only this context
  // workspace (one allocation)
  char* ws = nullptr;
  bf16_t *h, *xn, *qkv, *attn, *mlp, *cat, *ctx, *vout;
  bf16_t *tproj, *tmid, *te, *gproj, *gmid, *ge, *pmid, *pe, *temb, *st, *mods;
  float *cosT, *sinT, *ids, *tvals;
  // 8-bit modes: quantised activation rows + per-token scales (xq / xs: LayerNorm output, aq / as_: attention / MLP output)
  uint8_t *xq = nullptr, *aq = nullptr;
  float *xs = nullptr, *as_ = nullptr;
  char* attn_ws = nullptr;                  // hand-off workspace of the persistent attention kernel (contexts run concurrently)
  char* attn8_ws = nullptr;                 // packed e4m3 q | k | v^T of the 8-bit attention
  int attn_variant = 0;                     // 0: persistent (stream-K) joint attention; 1: one workgroup per (query tile, head) item
  bool shared_chip = false;                 // several images in flight (td_flux_denoise_multi): kernels of other contexts fill this one's empty rounds
  // History is the previous step's state OF THE SAME IMAGE UNDER THE SAME NUMERIC CONFIGURATION: set_condition / set_timesteps forget it, and
  // it is trusted only when recorded in the model's current hist_epoch.
  // 8-bit attention, history reference points (TdAttnParams::ref_in / ref_out): per (block, head, token) where the softmax of the NEXT denoise step
  // starts -- two buffers, read / written in turn (a launch reads one and max-accumulates into the other)
  int* href[2] = {nullptr, nullptr};
  int href_cur = 0, href_step = -1, href_T = 0, href_S = 0;      // href[href_cur] holds the references step `href_step` produced for this token layout
  int href_epoch = -1, hs_epoch = -1;       // the epoch href / hs_amax were recorded in
  // int8 with history scales (td_flux_set_act_scales): per (block tensor, token) the scale / inverse scale of THIS step, taken from the maxima the
  // previous step accumulated (hs_amax, float bits) -- tensors: MLP input of double block i = [i], [attn | mlp] operand of single block i = [L + i],
  // attention output of double block i = [L + Ls + i]
  float *hs_scale = nullptr, *hs_inv = nullptr;
  unsigned* hs_amax = nullptr;
  int hs_cap = 0;                           // tokens per tensor in the three arrays
  int hs_step = -1, hs_T = 0, hs_S = 0;     // the step (and token layout) whose maxima hs_amax holds
  std::vector<float> tv_host;               // host staging of the schedule scalars (td_flux_set_timesteps)
  int cond_epoch = 0, sched_epoch = 0;      // the model's weight_epoch at td_flux_set_condition / td_flux_set_timesteps
  // state
  int T = 0, S_img = 0, n_steps = 0;
  bool cond_set = false;
  // xin [max_img, Cin] is the operand of a channel-conditioned x_embedder: the latents are gathered into its first Cout columns at the head of
  // every forward, td_flux_set_channel_condition writes the rest once per image.  Ccond == 0: no xin, the forward reads the caller's latents.
  bf16_t* xin = nullptr;
  bool ccond_set = false;
  // reference tokens (FLUX.1 Kontext): S_ref rows that join the image stream behind the S_img latent rows in every forward, constant over the
  // schedule, never stepped or returned.  xref [max_img, Cout] is the operand of x_embedder while S_ref > 0: rows S_img .. S_img + S_ref are
  // written once per image (td_flux_set_reference_tokens), the head rows take the caller's latents by one device-to-device copy per forward.
  // The blocks then run over T + S_img + S_ref rows; the final norm, proj_out, the velocity and every step kernel keep S_img.
  int S_ref = 0;
  bf16_t* xref = nullptr;
  // ---- ControlNet.  On a ControlNet context (m->controlnet): the control mode (-1: none), E = controlnet_x_embedder(control latents) of the
  // image [max_img, D] -- the residual of every forward's x_embedder epilogue -- and the arena of UNSCALED samples the last forward left,
  // [n_d + n_s][max_img, D] (sample k at cn_samples + k * max_img * D).  cn_owner: the main context it is attached to (one at a time).
  int cn_mode_id = -1;
  bf16_t *cn_E = nullptr, *cn_samples = nullptr;
  bool cn_cond_set = false;
  td_flux* cn_owner = nullptr;
  // On a main context: the attached ControlNet contexts cns[0 .. n_cn) in list order (td_flux_attach_controlnets) and, per net, the conditioning
  // scale of every prepared step (host floats; missing entries are 1.0)
  td_flux* cns[TD_MAX_CONTROLNETS] = {};
  int n_cn = 0;
  std::vector<float> cn_scales[TD_MAX_CONTROLNETS];
  // ---- IP-Adapter: per slot the image-prompt tokens of THIS image and every double block's K / V of them (td_flux_set_ip_image_embeds; one
  // allocation per slot, made at first use and grown when a later call needs more): staging [n_img, E_pad] | projection [n_img, num_tokens J] |
  // tokens [n_keys, J] | kv [L][K, V][keys_pad][D] (rows n_keys .. keys_pad zero).  ip_out [max_img, D]: the sum over the active slots of one
  // block, written by td_ip_attention before the block's RoPE and added to the image rows behind its FF (first use as well).
  struct IpCtx {
    bool set = false;
    int n_img = 0, n_keys = 0, keys_pad = 0, epoch = -1;
    char* buf = nullptr;
    int64_t bytes = 0;
    bf16_t *stage = nullptr, *projd = nullptr, *tokens = nullptr, *kv = nullptr;
  };
  IpCtx ip[TD_IP_MAX_ADAPTERS];
  bf16_t* ip_out = nullptr;
  // ---- First-block cache state of THIS image (the settings are the model's).  One allocation, made at the first forward under the cache:
  // bc_r[2] [max_img, D] -- bc_r[bc_cur] is r_prev, the residual of the last computed forward, the other one receives this forward's -- and bc_tail
  // [max_img, D]: h1's latent rows during a computed forward, then (in place) what the remaining blocks added to them; bc_ws / bc_sums: the head
  // kernel's partial sums and its two fp64 results, which bc_host (16 pinned bytes) receives before the decision.  h0 needs no buffer of its own: it
  // waits in f->cat, which no double block touches.
  char* bc_buf = nullptr;
  bf16_t *bc_r[2] = {nullptr, nullptr}, *bc_tail = nullptr;
  double *bc_ws = nullptr, *bc_sums = nullptr, *bc_host = nullptr;
  int bc_cur = 0;
  bool bc_has_prev = false;                 // bc_r[bc_cur] and bc_tail hold a computed forward's values for the layout / epochs below
  int bc_T = 0, bc_S_img = 0, bc_S_ref = 0, bc_wepoch = -1, bc_cepoch = -1;
  int bc_count = 0;                         // forwards since the last reset (the schedule's index)
  std::vector<float> bc_metric;             // the log since the last reset (td_flux_block_cache_stats), at most BC_LOG_MAX entries
  std::vector<unsigned char> bc_computed;
  // optional per-launch HIP-event trace (bench.py roofline leg)
  bool tracing = false;
  std::vector<hipEvent_t> ev_pool;
  struct TraceRec { int cat; double flops; };
  std::vector<TraceRec> trace;
};
