// Host-side building blocks shared by the VAE decoder (vae_engine.hip) and encoder (vae_encoder.hip) engines: the weight-arena
// plan, the diffusers parameter table, ResnetBlock2D and the single-head mid-block attention on the GEMM / row kernels.
// The handle types (td_vae, td_vae_enc) are different structs with the same member names, hence the templates.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "td_kernels.h"
#include "../../include/thinkdiff_hip.h"

namespace tdvae {

struct VSlot { std::string name; bf16_t* ptr; int64_t count; int kind; int cout, cin, cout_pad, cin_pad; };  // kind 0 plain, 1 conv3x3

struct Resnet {
  int cin, cout;
  bf16_t *n1_w, *n1_b, *c1_w, *c1_b, *n2_w, *n2_b, *c2_w, *c2_b, *sc_w, *sc_b;
};

#define TDV_TRY(expr)         \
  do {                        \
    int _rc = (expr);         \
    if (_rc != 0) return _rc; \
  } while (0)

inline int pad64(int c) { return (c + 63) & ~63; }
inline int pad8(int c) { return (c + 7) & ~7; }

struct Plan {
  int64_t off = 0;
  std::vector<std::pair<bf16_t**, int64_t>> fix;
  void take(bf16_t** p, int64_t n) { fix.emplace_back(p, off); off += (n + 127) & ~int64_t(127); }
};

template <class F>
void v_add(F* f, const std::string& name, bf16_t* p, int64_t count, int kind = 0, int cout = 0, int cin = 0, int cout_pad = 0, int cin_pad = 0) {
  f->index[name] = (int)f->slots.size();
  f->slots.push_back({name, p, count, kind, cout, cin, cout_pad, cin_pad});
}

inline void plan_resnet(Plan& pl, Resnet& r, int cin, int cout) {
  r.cin = cin; r.cout = cout;
  pl.take(&r.n1_w, cin); pl.take(&r.n1_b, cin);
  pl.take(&r.c1_w, (int64_t)cout * 9 * cin); pl.take(&r.c1_b, cout);
  pl.take(&r.n2_w, cout); pl.take(&r.n2_b, cout);
  pl.take(&r.c2_w, (int64_t)cout * 9 * cout); pl.take(&r.c2_b, cout);
  r.sc_w = r.sc_b = nullptr;
  if (cin != cout) { pl.take(&r.sc_w, (int64_t)cout * cin); pl.take(&r.sc_b, cout); }
}

template <class F>
void name_resnet(F* f, const std::string& p, const Resnet& r) {
  v_add(f, p + "norm1.weight", r.n1_w, r.cin); v_add(f, p + "norm1.bias", r.n1_b, r.cin);
  v_add(f, p + "conv1.weight", r.c1_w, (int64_t)r.cout * r.cin * 9, 1, r.cout, r.cin, r.cout, r.cin);
  v_add(f, p + "conv1.bias", r.c1_b, r.cout);
  v_add(f, p + "norm2.weight", r.n2_w, r.cout); v_add(f, p + "norm2.bias", r.n2_b, r.cout);
  v_add(f, p + "conv2.weight", r.c2_w, (int64_t)r.cout * r.cout * 9, 1, r.cout, r.cout, r.cout, r.cout);
  v_add(f, p + "conv2.bias", r.c2_b, r.cout);
  if (r.sc_w) { v_add(f, p + "conv_shortcut.weight", r.sc_w, (int64_t)r.cout * r.cin, 0, r.cout, r.cin); v_add(f, p + "conv_shortcut.bias", r.sc_b, r.cout); }
}

// The single-head attention's parameters (Attention(heads=1) of UNetMidBlock2D)
struct MidAttn { bf16_t *gn_w, *gn_b, *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b; };

inline void plan_attn(Plan& pl, MidAttn& a, int c) {
  pl.take(&a.gn_w, c); pl.take(&a.gn_b, c);
  pl.take(&a.q_w, (int64_t)c * c); pl.take(&a.q_b, c);
  pl.take(&a.k_w, (int64_t)c * c); pl.take(&a.k_b, c);
  pl.take(&a.v_w, (int64_t)c * c); pl.take(&a.v_b, c);
  pl.take(&a.o_w, (int64_t)c * c); pl.take(&a.o_b, c);
}

template <class F>
void name_attn(F* f, const std::string& a, const MidAttn& m, int c) {
  v_add(f, a + "group_norm.weight", m.gn_w, c); v_add(f, a + "group_norm.bias", m.gn_b, c);
  v_add(f, a + "to_q.weight", m.q_w, (int64_t)c * c, 0, c, c); v_add(f, a + "to_q.bias", m.q_b, c);
  v_add(f, a + "to_k.weight", m.k_w, (int64_t)c * c, 0, c, c); v_add(f, a + "to_k.bias", m.k_b, c);
  v_add(f, a + "to_v.weight", m.v_w, (int64_t)c * c, 0, c, c); v_add(f, a + "to_v.bias", m.v_b, c);
  v_add(f, a + "to_out.0.weight", m.o_w, (int64_t)c * c, 0, c, c); v_add(f, a + "to_out.0.bias", m.o_b, c);
}

inline int conv3(hipStream_t s, const bf16_t* x, const bf16_t* w, const bf16_t* b, const bf16_t* res, bf16_t* y, int H, int W, int cin, int cout, int up) {
  TdGemmParams p;
  p.A = x; p.lda = cin; p.W = w; p.bias = b; p.C = y; p.ldc = cout; p.res = res; p.ldr = cout;
  p.M = H * W; p.N = cout; p.K = 9 * cin; p.conv_H = H; p.conv_W = W; p.conv_Cin = cin; p.conv_up = up;
  return td_gemm_launch(p, s);
}

inline int lin(hipStream_t s, const bf16_t* x, int ldx, const bf16_t* w, const bf16_t* b, bf16_t* y, int ldy, int M, int N, int K, const bf16_t* res = nullptr) {
  TdGemmParams p;
  p.A = x; p.lda = ldx; p.W = w; p.bias = b; p.C = y; p.ldc = ldy; p.M = M; p.N = N; p.K = K; p.res = res; p.ldr = ldy;
  return td_gemm_launch(p, s);
}

template <class F>
int gn(F* f, hipStream_t s, const bf16_t* x, bf16_t* y, int P, int C, const bf16_t* w, const bf16_t* b, int silu) {
  return td_groupnorm_nhwc_launch(x, y, P, C, f->cfg.norm_groups, 1e-6f, w, b, silu, f->gn, s);
}

// x (in X) -> X, using T1..T3;  ResnetBlock2D: x + conv2(silu(gn2(conv1(silu(gn1(x))))))  (shortcut 1x1 when cin != cout)
template <class F>
int resnet(F* f, hipStream_t s, const Resnet& r, int H, int W) {
  const int P = H * W;
  TDV_TRY(gn(f, s, f->X, f->T1, P, r.cin, r.n1_w, r.n1_b, 1));
  TDV_TRY(conv3(s, f->T1, r.c1_w, r.c1_b, nullptr, f->T2, H, W, r.cin, r.cout, 0));
  TDV_TRY(gn(f, s, f->T2, f->T1, P, r.cout, r.n2_w, r.n2_b, 1));
  const bf16_t* sc = f->X;
  if (r.sc_w) { TDV_TRY(lin(s, f->X, r.cin, r.sc_w, r.sc_b, f->T3, r.cout, P, r.cout, r.cin)); sc = f->T3; }
  TDV_TRY(conv3(s, f->T1, r.c2_w, r.c2_b, sc, f->X, H, W, r.cout, r.cout, 0));
  return 0;
}

// x (in X, [P0, c]) -> X + to_out(attention(gn(x))), using T1, T2, Q, K, VT, S, P.  ONE head of width c: scores are produced in fp32
// row chunks of f->chunk_rows by the GEMM (fp32 output), softmaxed by a row kernel and multiplied with V^T by the GEMM again; to_v's
// bias is added after the product (softmax rows sum to 1).
// The P . V^T product contracts over the keys and the GEMM's K must be a multiple of 64: the KEY axis of S / P / V^T is padded to
// Pk = pad64(P0).  The pad rows of gn(x) are zeroed in every call (T1 is a scratch buffer other stages write), so V^T's pad columns are exact
// zeros (to_v runs without its bias here): that is the memset correctness rests on.  K's pad rows are zeroed only to keep uninitialised memory
// out of the score GEMM -- the score columns they produce are never read; the softmax normalises over the P0 real columns and writes
// zeros into P's pad columns, and 0 x 0 adds nothing to the fp32 accumulator.  With P0 % 64 == 0 there is no pad: the launches, their extents and every bit are those of the unpadded form.
template <class F>
int mid_attention(F* f, hipStream_t s, const MidAttn& a, int P0, int c) {
  const int Pk = pad64(P0);
  TDV_TRY(gn(f, s, f->X, f->T1, P0, c, a.gn_w, a.gn_b, 0));
  if (Pk != P0) {
    TD_CHECK_HIP(hipMemsetAsync(f->T1 + (size_t)P0 * c, 0, (size_t)(Pk - P0) * c * sizeof(bf16_t), s));
    TD_CHECK_HIP(hipMemsetAsync(f->K + (size_t)P0 * c, 0, (size_t)(Pk - P0) * c * sizeof(bf16_t), s));
  }
  TDV_TRY(lin(s, f->T1, c, a.q_w, a.q_b, f->Q, c, P0, c, c));
  TDV_TRY(lin(s, f->T1, c, a.k_w, a.k_b, f->K, c, P0, c, c));
  TDV_TRY(lin(s, a.v_w, c, f->T1, nullptr, f->VT, Pk, c, Pk, c));      // V^T [c, Pk] = Wv . xn^T (bias added after PV)
  const float scale = 1.0f / sqrtf((float)c);
  for (int r0 = 0; r0 < P0; r0 += f->chunk_rows) {
    const int rows = std::min(f->chunk_rows, P0 - r0);
    TdGemmParams g;   // scores (fp32) = Q_chunk . K^T
    g.A = f->Q + (size_t)r0 * c; g.lda = c; g.W = f->K; g.C = (bf16_t*)f->S; g.ldc = Pk; g.M = rows; g.N = Pk; g.K = c; g.out_f32 = 1;
    g.cfg = Pk <= 64 ? 1 : (rows <= 32 ? 2 : 0);
    TDV_TRY(td_gemm_launch(g, s));
    TDV_TRY(td_softmax_rows_launch(f->S, f->P, rows, P0, Pk, scale, s));
    TDV_TRY(lin(s, f->P, Pk, f->VT, a.v_b, f->T2 + (size_t)r0 * c, c, rows, c, Pk));   // + b_v: softmax rows sum to 1
  }
  TDV_TRY(lin(s, f->T2, c, a.o_w, a.o_b, f->X, c, P0, c, c, f->X));   // to_out + residual
  return 0;
}

// ---- parameter table entry points (td_vae_* / td_vae_enc_*): `what` prefixes the error messages -------------------------------------
template <class F>
int param_info(const F* f, const char* what, int idx, char* name_buf, int buf_len, int64_t* count) {
  TD_CHECK_ARG(f && idx >= 0 && idx < (int)f->slots.size(), "%s: index %d out of range", what, idx);
  if (name_buf && buf_len > 0) { strncpy(name_buf, f->slots[idx].name.c_str(), buf_len - 1); name_buf[buf_len - 1] = 0; }
  if (count) *count = f->slots[idx].count;
  return TD_OK;
}

// src: device bf16 in the torch layout ([Cout,Cin,3,3] for 3x3 convs, [out,in(,1,1)] otherwise, [C] vectors)
template <class F>
int load_param(F* f, const char* what, const char* name, const void* src, int64_t count, void* stream) {
  TD_CHECK_ARG(f && name && src, "%s: null argument", what);
  auto it = f->index.find(name);
  TD_CHECK_ARG(it != f->index.end(), "%s: unknown parameter '%s'", what, name);
  const VSlot& s = f->slots[it->second];
  TD_CHECK_ARG(s.count == count, "%s: '%s' expects %lld elements, got %lld", what, name, (long long)s.count, (long long)count);
  if (s.kind == 1) return td_conv_pack_launch((const bf16_t*)src, s.ptr, s.cout, s.cin, s.cout_pad, s.cin_pad, (hipStream_t)stream);
  TD_CHECK_HIP(hipMemcpyAsync(s.ptr, src, (size_t)count * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return TD_OK;
}

template <class F>
int init_random(F* f, const char* what, uint64_t seed, float std, void* stream) {
  TD_CHECK_ARG(f, "%s: null handle", what);
  for (const VSlot& s : f->slots) {
    const bool norm_w = s.name.find("norm") != std::string::npos && s.name.find(".weight") != std::string::npos;
    const int64_t n = s.kind == 1 ? (int64_t)s.cout * 9 * s.cin_pad : s.count;   // padded output rows stay zero
    // std <= 0: variance-preserving weights (1 / sqrt(fan_in) for convolutions and linears, 0.02 for biases), so that a synthetic
    // decoder maps unit-scale latents to an image with contrast instead of a flat grey one
    float sd = std;
    if (std <= 0.f) sd = s.cin > 0 ? 1.0f / sqrtf((float)(s.kind == 1 ? 9 * s.cin : s.cin)) : 0.02f;
    TDV_TRY(td_fill_normal_bf16(s.ptr, n, seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(s.ptr - f->arena + 1)), norm_w ? 0.05f : sd, norm_w ? 1.0f : 0.0f, stream));
  }
  // padded input channels of conv_in get random weights too: their activations are zero
  return TD_OK;
}

}  // namespace tdvae
