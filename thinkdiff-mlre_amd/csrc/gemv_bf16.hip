// Skinny-M Linear for gfx950: y[M<=64, N] = epilogue(x[M,K] . W[N,K]^T), the weight-streaming case of the hot path --
// KV-cached Qwen2-VL decode (one token against 7.6 B parameters: SURVEY.md 8a row A7, HBM roofline), the pooled / timestep
// embedders of FLUX, lm_head.  The MFMA tile kernel launches N/256 workgroups here (14 for down_proj) and leaves the
// chip idle; this kernel is a plain HBM stream:
//   * a workgroup (4 waves) owns 4 consecutive output columns = 4 weight rows; its 256 threads stride the rows' 16-byte
//     chunks, so every wave-level load is a fully coalesced 1 KiB line run; loads are non-temporal (weights are read once);
//   * two chunk-columns are in flight per thread (8 weight loads + the matching x chunks, which hit L2);
//   * bf16 pairs go straight into v_dot2c_f32_bf16 (fp32 accumulate, no unpacking); the W8 / W4 forms stream e4m3 bytes / MXFP4 nibbles and convert them
//     to those pairs in one instruction per pair (csrc/e4m3_pow2.h, csrc/mxfp4_pow2.h); the I4 form streams the uint4 nibbles of AWQ / GPTQ checkpoints and
//     rebuilds the pairs with one fp32 fma per weight and one rounding (csrc/int4_group.h);
//   * wave shuffle + LDS cross-wave reduction, then the same epilogue semantics and bf16 rounding points as the tile kernel
//     (bias, activation, gate, residual, split output).
#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "td_common.h"
#include "td_kernels.h"
#include "e4m3_pow2.h"
#include "mxfp4_pow2.h"
#include "int4_group.h"

namespace {

__device__ __forceinline__ float act_rt(int act, float x) {
  switch (act) {
    case TD_ACT_GELU_TANH: return gelu_tanh_f(x);
    case TD_ACT_GELU_ERF: return gelu_erf_f(x);
    case TD_ACT_SILU: return silu_f(x);
    case TD_ACT_QUICK_GELU: return quick_gelu_f(x);
    default: return x;      // TD_ACT_NONE (td_gemm_launch refuses unknown codes)
  }
}

// 8-bit weights (TdGemmParams::W8, the format of csrc/e4m3_pow2.h): 16 bytes of a row -> 8 bf16 pairs with the row's scale, so v_dot2c sees the
// operands it sees on the bf16 path
__device__ __forceinline__ void cvt16(const u32x4_t& w, float scale, u32x4_t& lo, u32x4_t& hi) {
  lo = e4m3p2_to_bf16(u32x2_t{w[0], w[1]}, scale);
  hi = e4m3p2_to_bf16(u32x2_t{w[2], w[3]}, scale);
}

constexpr int R = 4;          // weight rows (output columns) per workgroup
constexpr int THREADS = 256;

// what the weight rows of a stream kernel hold (the WF template parameter): bf16 values, e4m3 bytes under a row scale (TdGemmParams::W8), or MXFP4
// nibbles under a scale byte per 32 weights (TdGemmParams::W4), or uint4 nibbles under an fp16 scale and a zero point per group (TdGemmParams::I4)
constexpr int WF_BF16 = 0, WF_W8 = 1, WF_W4 = 2, WF_I4 = 3;
// the argument block of a form's kernels: only I4 reads (and carries) the int4 fields of TdGemmParams
template <int WF> using GemvArgs = std::conditional_t<WF == WF_I4, TdGemmParams, TdGemmArgs>;

// W8: the weight rows are e4m3 bytes (p.W8, p.w8_scale); a 16-byte chunk then holds 16 weights and meets two chunks of x.  Everything behind the
// accumulators is shared with the bf16 form.
// W4: the weight rows are MXFP4 nibbles (p.W4, p.w4_scale; the format of csrc/mxfp4_pow2.h); a 16-byte chunk is then exactly one MX block: 32 weights
// under one scale byte, which the thread loads beside the chunk, and meets four chunks of x.  The chunk is converted a dword (8 weights) at a time.
// I4: the weight rows are grouped int4 nibbles (p.I4, p.i4_scale, p.i4_zero, p.i4_gshift; the format of csrc/int4_group.h).  The loop is the W4 loop: a 16-byte
// chunk is 32 weights inside ONE group, whose fp16 scale and zero point the thread loads beside the chunk and combines once (i4_group).
template <int MR, int WF = WF_BF16>
__global__ __launch_bounds__(THREADS) void td_gemv_bf16_kernel(const GemvArgs<WF> p) {
  constexpr bool W8 = WF == WF_W8, W4 = WF == WF_W4, I4 = WF == WF_I4;
  __shared__ float red[THREADS / 64][R][MR];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n0 = blockIdx.x * R;
  const int nchunk = (W4 || I4) ? p.K >> 5 : W8 ? p.K >> 4 : p.K >> 3;
  const u32x4_t* wp[R];
  const uint8_t* sp[R];      // W4: the row's scale bytes, one per chunk
  const uint16_t* isp[R];    // I4: the row's group scales and zero points, one per (chunk >> gsh)
  const uint8_t* izp[R];
  int gsh = 0;
  if constexpr (I4) gsh = p.i4_gshift - 5;
  float wsc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    // gated mode: rows 0,1 = gate rows 2b, 2b+1; rows 2,3 = the matching up rows (glu_I further down the matrix)
    const int row = p.glu_I ? (blockIdx.x * 2 + (r & 1) + (r >> 1) * p.glu_I) : min(n0 + r, p.N - 1);
    sp[r] = nullptr; isp[r] = nullptr; izp[r] = nullptr;
    if constexpr (I4) {
      wp[r] = (const u32x4_t*)(p.I4 + (size_t)row * (p.K >> 1));
      isp[r] = p.i4_scale + (size_t)row * (p.K >> p.i4_gshift);
      izp[r] = p.i4_zero + (size_t)row * (p.K >> p.i4_gshift);
      wsc[r] = 1.f;
    } else if constexpr (W4) {
      wp[r] = (const u32x4_t*)(p.W4 + (size_t)row * (p.K >> 1));
      sp[r] = p.w4_scale + (size_t)row * (p.K >> 5);
      wsc[r] = 1.f;
    } else if constexpr (W8) {
      wp[r] = (const u32x4_t*)(p.W8 + (size_t)row * p.K);
      wsc[r] = p.w8_scale[row];
    } else {
      wp[r] = (const u32x4_t*)(p.W + (size_t)row * p.K);
      wsc[r] = 1.f;
    }
  }
  const u32x4_t* xp[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) xp[m] = (const u32x4_t*)(p.A + (size_t)min(m, p.M - 1) * p.lda);

  float acc[R][MR];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[r][m] = 0.f;

  // W4 / I4: one chunk (= one block; inside one group) of the R rows, at chunk index cc, against its four chunks of x; sb: the scale byte / the group
  auto eat4 = [&](const u32x4_t (&w)[R], const auto (&sb)[R], int cc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4_t a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if constexpr (I4) a[r] = i4_to_bf16(w[r][i], sb[r]);
        else a[r] = mx4_to_bf16(w[r][i], mx4_scale_f32(sb[r]));
      }
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const u32x4_t x = xp[m][4 * cc + i];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][m] = dot8(a[r], x, acc[r][m]);
      }
    }
  };

  int c = tid;
  for (; c + THREADS < nchunk; c += 2 * THREADS) {
    u32x4_t w0[R], w1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      w0[r] = __builtin_nontemporal_load(wp[r] + c);
      w1[r] = __builtin_nontemporal_load(wp[r] + c + THREADS);
    }
    if constexpr (I4) {
      I4Group g0[R], g1[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int e0 = c >> gsh, e1 = (c + THREADS) >> gsh;
        g0[r] = i4_group(isp[r][e0], izp[r][e0]);
        g1[r] = i4_group(isp[r][e1], izp[r][e1]);
      }
      eat4(w0, g0, c);
      eat4(w1, g1, c + THREADS);
    } else if constexpr (W4) {
      unsigned s0[R], s1[R];
#pragma unroll
      for (int r = 0; r < R; ++r) { s0[r] = sp[r][c]; s1[r] = sp[r][c + THREADS]; }
      eat4(w0, s0, c);
      eat4(w1, s1, c + THREADS);
    } else if constexpr (W8) {
      u32x4_t a0[R], b0[R], a1[R], b1[R];
#pragma unroll
      for (int r = 0; r < R; ++r) { cvt16(w0[r], wsc[r], a0[r], b0[r]); cvt16(w1[r], wsc[r], a1[r], b1[r]); }
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const u32x4_t x0 = xp[m][2 * c], x1 = xp[m][2 * c + 1], x2 = xp[m][2 * (c + THREADS)], x3 = xp[m][2 * (c + THREADS) + 1];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][m] = dot8(b1[r], x3, dot8(a1[r], x2, dot8(b0[r], x1, dot8(a0[r], x0, acc[r][m]))));
      }
    } else {
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const u32x4_t x0 = xp[m][c], x1 = xp[m][c + THREADS];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][m] = dot8(w1[r], x1, dot8(w0[r], x0, acc[r][m]));
      }
    }
  }
  if (c < nchunk) {
    u32x4_t w0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) w0[r] = __builtin_nontemporal_load(wp[r] + c);
    if constexpr (I4) {
      I4Group g0[R];
#pragma unroll
      for (int r = 0; r < R; ++r) g0[r] = i4_group(isp[r][c >> gsh], izp[r][c >> gsh]);
      eat4(w0, g0, c);
    } else if constexpr (W4) {
      unsigned s0[R];
#pragma unroll
      for (int r = 0; r < R; ++r) s0[r] = sp[r][c];
      eat4(w0, s0, c);
    } else if constexpr (W8) {
      u32x4_t a0[R], b0[R];
#pragma unroll
      for (int r = 0; r < R; ++r) cvt16(w0[r], wsc[r], a0[r], b0[r]);
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const u32x4_t x0 = xp[m][2 * c], x1 = xp[m][2 * c + 1];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][m] = dot8(b0[r], x1, dot8(a0[r], x0, acc[r][m]));
      }
    } else {
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const u32x4_t x0 = xp[m][c];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][m] = dot8(w0[r], x0, acc[r][m]);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const float v = wave_sum(acc[r][m]);
      if (lane == 0) red[wid][r][m] = v;
    }
  __syncthreads();
  if (p.glu_I) {
    if (tid >= 2 * MR) return;
    const int i = tid / MR, m = tid % MR;
    if (m >= p.M) return;
    float gsum = 0.f, usum = 0.f;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) { gsum += red[w][i][m]; usum += red[w][i + 2][m]; }
    p.C[(size_t)m * p.ldc + blockIdx.x * 2 + i] = f2bf(rbf(silu_f(rbf(gsum))) * rbf(usum));
    return;
  }
  if (tid >= R * MR) return;
  const int r = tid / MR, m = tid % MR;
  const int n = n0 + r;
  if (n >= p.N || m >= p.M) return;
  float v = 0.f;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) v += red[w][r][m];
  // epilogue: the tile kernel's semantics and rounding points (Linear output, activation, gate, residual each round)
  const bool second = p.C2 != nullptr && n >= p.n_split;
  const int act = second ? p.act2 : p.act;
  if (p.bias) v += bf2f(p.bias[n]);
  if (act != TD_ACT_NONE) v = act_rt(act, rbf(v));
  if (p.gate) v = rbf(v) * bf2f(p.gate[n]);
  if (p.res) v = rbf(v) + bf2f(p.res[(size_t)m * p.ldr + n]);
  if (second) p.C2[(size_t)m * p.ldc2 + (n - p.n_split)] = f2bf(v);
  else p.C[(size_t)m * p.ldc + n] = f2bf(v);
}

// ---- 4 < M <= 64: the same weight stream on the matrix core ---------------------------------------------------------
// With more activation rows the dot-product form re-reads x from L2 MR times per weight chunk (at M = 16 x traffic is 8x the
// weight traffic and the kernel stops scaling).  Here a workgroup owns NR blocks of 16 weight rows, its 8 waves split K in
// 64-element steps, and every step is two v_mfma_f32_16x16x32_bf16 per (weight block, activation block) with the weight rows as
// the A operand and 16 activation rows as the B operand -- both fragments are loaded straight from global memory in MFMA operand
// layout (lane = row, 16 B of k), so there is no VALU work in the loop.  MB = ceil(M / 16) activation blocks share every weight
// fragment (batched decode of up to 64 sequences: one pass over the weights); x comes from L2, MB / NR bytes per weight byte.
// Accumulators are reduced across waves through LDS, one weight block at a time.
constexpr int MW = 8;   // waves per workgroup (K split)

// Few weight blocks (N = hidden: 96 blocks for the 2B decoder, 224 for the 7B one) leave most CUs without a workgroup.  Then K is
// also split across KS workgroups per block column (gridDim.y): each leaves its fp32 partial tiles in a workspace and draws a
// ticket; the LAST to arrive adds the KS partials in index order (the result does not depend on who finishes) and runs the epilogue.
// Hand-off as in the stream-K attention kernel: write-through (sc1) 16-byte stores, every storing wave drains, workgroup barrier,
// one agent-scope atomic; reader: one agent-scope acquire, barrier, plain loads.  The finisher re-arms the counter.
constexpr int SPLITK_MAX_WGS = 512;                       // block columns a split launch may have (sizes the counter array)
constexpr size_t SPLITK_HEADER_BYTES = SPLITK_MAX_WGS * 4;
constexpr size_t SPLITK_PART_BYTES = (size_t)SPLITK_MAX_WGS * 4 * 8 * 1024;   // block columns x MB x KS x (64 lanes x 16 B)

// LDS bytes of one workgroup: per wave a private slab of 2 NR weight + 2 XB activation 1-KiB fragments (one k-step; more than two
// activation blocks take turns in the slab, which keeps 2-3 workgroups per CU at 64 sequences), reused for the cross-wave
// reduction (MB KiB per wave) after the loop
template <int MB> constexpr int gemv_xb() { return MB > 2 ? 2 : MB; }     // activation blocks passing through the slab together
template <int MB, int NR> constexpr int gemv_lds_bytes() { return MW * (2 * NR + 2 * gemv_xb<MB>()) * 1024; }

// W8 (TdGemmParams::W8): the weight rows are e4m3 bytes.  A whole 128-byte line of a row is then 128 weights, so a step covers 128 elements of K: the same
// two weight loads per block as a bf16 step (8 rows x one line each), twice the activation loads, and the loop body below runs its two 64-element halves
// in turn.  The weight lines go through the slab AS BYTES (same writes, same XOR placement of the 16-byte chunks); a lane reads the 8 bytes of its operand
// fragment back (ds_read_b64) and converts them with its row's scale (e4m3p2_to_bf16) into the very bf16 fragment the bf16
// form would have read.  Accumulators, reduction, split-K hand-off and epilogue are shared.
// W4 (TdGemmParams::W4): the weight rows are MXFP4 nibbles.  A 128-byte line of a row is 256 weights = 8 MX blocks, so a step covers 256 elements of K: the
// same two weight loads per block, four times the activation loads, four 64-element quarters in turn.  A lane's 8-element operand fragment is 4 bytes
// (ds_read_b32) inside ONE 16-byte chunk = one block, so one scale per fragment: the 8 scale bytes of the lane's row and step arrive in one 8-byte load
// in operand layout (lane = row r) beside the weight lines, and mx4_to_bf16 rebuilds the bf16 fragment.
// I4 (TdGemmParams::I4): the weight rows are grouped int4 nibbles; lines, steps, slab and fragments are those of W4.  A fragment lies in one 16-byte chunk and
// therefore in one group: the 256 / G groups of the lane's row and step -- their fp16 scales in one load of 4 .. 16 bytes, their zero points in one of
// 2 .. 8 -- arrive beside the weight lines, and i4_to_bf16 rebuilds the bf16 fragment with the single rounding of csrc/int4_group.h.  The group size is a
// kernel argument: the loads and a byte permute that spreads the groups over the line's 8 chunks run under a uniform branch, everything behind is one code.
template <int MB, int NR, bool DEEP, int WF = WF_BF16>
__global__ __launch_bounds__(MW * 64) void td_gemv_mfma_kernel(const GemvArgs<WF> p, char* ws) {
  constexpr bool W8 = WF == WF_W8, W4 = WF == WF_W4, I4 = WF == WF_I4, N4 = W4 || I4;      // N4: nibble rows
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int XB = gemv_xb<MB>();
  constexpr int SLAB = (2 * NR + 2 * XB) * 1024;
  float (*red)[SLAB / 4] = (float (*)[SLAB / 4])smem;        // red[wave][(mb * 64 + lane) * 4 + i], MB KiB of each wave's slab
  __shared__ unsigned ticket_lds;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int nblk = p.glu_I ? p.glu_I / 8 : p.N / 16;         // 16-row weight blocks of the problem
  const int KS = gridDim.y, ky = blockIdx.y;
  // Operands through buffer descriptors: a k-step past this workgroup's range is sent beyond the descriptor and reads zeros, so
  // the loop body is branch-free.  A load instruction covers 8 rows x one whole 128-byte line each (lane = row l / 8, 16-byte chunk
  // l % 8): in MFMA operand layout (4 lanes per row) it would touch 16 half lines, and the other halves, fetched by the next
  // instruction, no longer find their lines in the 16 KiB L1 -- measured with a timing-only build: -17 % (16 sequences) to -27 %
  // (64) per decode step.  The fragments then pass through a wave-private LDS slab into operand layout: ds_write_b128 at lane x 16
  // (conflict-free), ds_read_b128 of row r, chunk 4 h + g; the chunk a lane FETCHES is XOR-ed with its row so those reads spread
  // over the banks.  LDS operations of a wave execute in order, so the slab needs no barrier between steps.
  // DEEP (long K: at least 4 steps per wave): all loads of SF steps -- up to 32 per lane -- are in flight before the first
  // LDS pass (a workgroup streams only 16 rows x K, its lifetime is a handful of memory round trips); otherwise hipcc threads
  // the loads between the steps at low register count, which keeps several workgroups per CU for short K.
  const unsigned w_rows = p.glu_I ? 2u * (unsigned)p.glu_I : (unsigned)p.N;
  const void* nib = p.W4;      // the nibble rows of either 4-bit form
  if constexpr (I4) nib = p.I4;
  const __amdgpu_buffer_rsrc_t rsW = N4   ? __builtin_amdgcn_make_buffer_rsrc((void*)nib, 0, (unsigned)((size_t)w_rows * (p.K >> 1)), 0x00020000)
                                     : W8 ? __builtin_amdgcn_make_buffer_rsrc((void*)p.W8, 0, (unsigned)((size_t)w_rows * p.K), 0x00020000)
                                          : __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (unsigned)((size_t)w_rows * p.K * 2), 0x00020000);
  // W4: the scale bytes [w_rows, K / 32]; a lane reads the 8 of its operand row and step (K % 256 == 0: 8-byte aligned)
  const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void*)p.w4_scale, 0, W4 ? (unsigned)((size_t)w_rows * (p.K >> 5)) : 0u, 0x00020000);
  // I4: the fp16 scales and the zero points [w_rows, K / G]; a lane reads the 256 / G of its operand row and step (K % 256 == 0: naturally aligned)
  int gsh = 0;      // chunks per group, as a shift
  __amdgpu_buffer_rsrc_t rsIS = rsS, rsIZ = rsS;
  if constexpr (I4) {
    gsh = p.i4_gshift - 5;
    rsIS = __builtin_amdgcn_make_buffer_rsrc((void*)p.i4_scale, 0, (unsigned)((size_t)w_rows * (p.K >> p.i4_gshift) * 2), 0x00020000);
    rsIZ = __builtin_amdgcn_make_buffer_rsrc((void*)p.i4_zero, 0, (unsigned)((size_t)w_rows * (p.K >> p.i4_gshift)), 0x00020000);
  }
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (unsigned)((((size_t)p.M - 1) * p.lda + p.K) * 2), 0x00020000);
  constexpr unsigned OOB = 0xFFFFFF00u;
  const int lrow = lane >> 3;                                  // row of the 8-row half this lane fetches
  const int lchunk = (lane & 7) ^ (lrow & 7);                  // ... and which 16-byte chunk of the row's 128-byte line
  unsigned woff[NR][2], xoff[MB][2];
  float wsc[NR];                                               // W8: scale of the weight row this lane holds in operand layout (row r of the block)
  unsigned soff[NR];                                           // W4: where that row's scale bytes begin; I4: its first group
#pragma unroll
  for (int nr = 0; nr < NR; ++nr) {
    const int bid = min((int)blockIdx.x * NR + nr, nblk - 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // gated mode: rows 0-7 = gate rows 8b..8b+7, rows 8-15 = the matching up rows
      const int wr_ = p.glu_I ? (bid * 8 + lrow + h * p.glu_I) : bid * 16 + 8 * h + lrow;
      woff[nr][h] = N4   ? (unsigned)((size_t)wr_ * (p.K >> 1) + 16 * lchunk)
                    : W8 ? (unsigned)((size_t)wr_ * p.K + 16 * lchunk)
                         : (unsigned)(((size_t)wr_ * p.K + 8 * lchunk) * 2);
    }
    const int orow = p.glu_I ? (bid * 8 + (r & 7) + (r >> 3) * p.glu_I) : bid * 16 + r;      // the weight row this lane holds in operand layout
    if constexpr (W8) wsc[nr] = p.w8_scale[orow];
    else wsc[nr] = 1.f;
    soff[nr] = W4 ? (unsigned)((size_t)orow * (p.K >> 5)) : 0u;
    if constexpr (I4) soff[nr] = (unsigned)((size_t)orow * (p.K >> p.i4_gshift));
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int h = 0; h < 2; ++h) xoff[mb][h] = (unsigned)(((size_t)min(16 * mb + 8 * h + lrow, p.M - 1) * p.lda + 8 * lchunk) * 2);
  char* slab = smem + wid * SLAB;
  u32x4_t* wr_ptr = (u32x4_t*)(slab + lane * 16);                                 // + fragment * 1024
  const char* rd_ptr[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) rd_ptr[h] = slab + r * 128 + (((4 * h + g) ^ (r & 7)) << 4);   // + block * 2048
  // W8: bytes of the 8 fragment bytes of (half j of the step, h): k = 64 j + 32 h + 8 g .. + 7 = chunk 4 j + 2 h + g / 2 of the row's line, its half g % 2
  const char* rd8_ptr[2][2];
  if constexpr (W8) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) rd8_ptr[j][h] = slab + r * 128 + (((4 * j + 2 * h + (g >> 1)) ^ (r & 7)) << 4) + 8 * (g & 1);
  }
  // W4: the 4 fragment bytes of (quarter j of the step, h): k = 64 j + 32 h + 8 g .. + 7 = chunk (= block) 2 j + h of the row's line, its bytes 4 g .. 4 g + 3
  const char* rd4_ptr[4][2];
  if constexpr (N4) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) rd4_ptr[j][h] = slab + r * 128 + (((2 * j + h) ^ (r & 7)) << 4) + 4 * g;
  }
  constexpr int KH = N4 ? 4 : W8 ? 2 : 1;       // 64-element parts of a step
  const int nk_all = N4 ? p.K >> 8 : W8 ? p.K >> 7 : p.K >> 6;  // steps (64 elements; W8: 128; W4: 256)
  const int s_beg = (int)((long long)nk_all * ky / KS), nk = (int)((long long)nk_all * (ky + 1) / KS);   // this workgroup's steps
  f32x4_t acc[NR][MB];
#pragma unroll
  for (int nr = 0; nr < NR; ++nr)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[nr][mb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  constexpr int SF = DEEP ? (32 / (2 * NR + 2 * KH * MB) > 0 ? 32 / (2 * NR + 2 * KH * MB) : 1) : (MB * NR == 1 ? 2 : 1);    // k-steps per wave and iteration
  for (int s = s_beg + wid; s < nk; s += SF * MW) {
    u32x4_t w[SF][NR][2], x[SF][KH][MB][2];
    u32x2_t sc4[SF][NR];      // W4: the step's 8 scale bytes of the lane's operand row
    u32x4_t si4[SF][NR];      // I4: the step's 8 >> gsh group scales of that row (fp16 bits, two to a word) ...
    u32x2_t zi4[SF][NR];      // ... and zero points (four to a word)
#pragma unroll
    for (int f = 0; f < SF; ++f) {
      const int st = s + f * MW;
      const bool ok = st < nk;
      const unsigned k0 = (unsigned)st * 128u;      // a step is one 128-byte line of every weight row in both forms
#pragma unroll
      for (int nr = 0; nr < NR; ++nr)
#pragma unroll
        for (int h = 0; h < 2; ++h) w[f][nr][h] = __builtin_amdgcn_raw_buffer_load_b128(rsW, ok ? woff[nr][h] + k0 : OOB, 0, 0);
      if constexpr (W4) {
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) sc4[f][nr] = __builtin_amdgcn_raw_buffer_load_b64(rsS, ok ? soff[nr] + (unsigned)st * 8u : OOB, 0, 0);
      }
      if constexpr (I4) {
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) {
          const unsigned e0 = soff[nr] + ((unsigned)st << (3 - gsh));      // the step's first group of the row
          si4[f][nr] = u32x4_t{0u, 0u, 0u, 0u};
          zi4[f][nr] = u32x2_t{0u, 0u};
          if (gsh == 2) {
            si4[f][nr][0] = __builtin_amdgcn_raw_buffer_load_b32(rsIS, ok ? e0 * 2u : OOB, 0, 0);
            zi4[f][nr][0] = __builtin_amdgcn_raw_buffer_load_b16(rsIZ, ok ? e0 : OOB, 0, 0);
          } else if (gsh == 1) {
            const u32x2_t t = __builtin_amdgcn_raw_buffer_load_b64(rsIS, ok ? e0 * 2u : OOB, 0, 0);
            si4[f][nr][0] = t[0]; si4[f][nr][1] = t[1];
            zi4[f][nr][0] = __builtin_amdgcn_raw_buffer_load_b32(rsIZ, ok ? e0 : OOB, 0, 0);
          } else {
            si4[f][nr] = __builtin_amdgcn_raw_buffer_load_b128(rsIS, ok ? e0 * 2u : OOB, 0, 0);
            zi4[f][nr] = __builtin_amdgcn_raw_buffer_load_b64(rsIZ, ok ? e0 : OOB, 0, 0);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < KH; ++j)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int h = 0; h < 2; ++h) x[f][j][mb][h] = __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? xoff[mb][h] + KH * k0 + 128u * j : OOB, 0, 0);
    }
    if (DEEP) __builtin_amdgcn_sched_barrier(0);   // hipcc otherwise threads the loads between the steps and keeps 4-6 of them in flight
#pragma unroll
    for (int f = 0; f < SF; ++f) {
      // block b of the slab: fragments 2b (rows 0-7) and 2b + 1 (rows 8-15); weight blocks first, then activation blocks
#pragma unroll
      for (int nr = 0; nr < NR; ++nr)
#pragma unroll
        for (int h = 0; h < 2; ++h) wr_ptr[(2 * nr + h) * 64] = w[f][nr][h];
      if constexpr (I4) {      // spread the step's 8 >> gsh groups over the 8 chunks of the line: from here on chunk j reads half j / byte j, whatever G is
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) {
          const unsigned s0 = si4[f][nr][0], s1 = si4[f][nr][1], z = zi4[f][nr][0];
          if (gsh == 2) {
            const unsigned a = __builtin_amdgcn_perm(s0, s0, 0x01000100u), b = __builtin_amdgcn_perm(s0, s0, 0x03020302u);
            si4[f][nr] = u32x4_t{a, a, b, b};
            zi4[f][nr] = u32x2_t{__builtin_amdgcn_perm(z, z, 0x00000000u), __builtin_amdgcn_perm(z, z, 0x01010101u)};
          } else if (gsh == 1) {
            si4[f][nr] = u32x4_t{__builtin_amdgcn_perm(s0, s0, 0x01000100u), __builtin_amdgcn_perm(s0, s0, 0x03020302u),
                                 __builtin_amdgcn_perm(s1, s1, 0x01000100u), __builtin_amdgcn_perm(s1, s1, 0x03020302u)};
            zi4[f][nr] = u32x2_t{__builtin_amdgcn_perm(z, z, 0x01010000u), __builtin_amdgcn_perm(z, z, 0x03030202u)};
          }
        }
      }
#pragma unroll
      for (int kh = 0; kh < KH; ++kh) {
      bf16x8_t wf[NR][2];
#pragma unroll
      for (int m0 = 0; m0 < MB; m0 += XB) {       // XB activation blocks at a time through the slab
#pragma unroll
        for (int j = 0; j < XB; ++j)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            if (m0 + j < MB) wr_ptr[(2 * (NR + j) + h) * 64] = x[f][kh][m0 + j < MB ? m0 + j : 0][h];
        bf16x8_t xf[XB][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (m0 == 0) {
#pragma unroll
            for (int nr = 0; nr < NR; ++nr) {
              if constexpr (I4) {
                const int j = 2 * kh + h;                                                          // chunk of the line
                const unsigned sb = (si4[f][nr][j >> 1] >> (16 * (j & 1))) & 0xffffu, zb = (zi4[f][nr][j >> 2] >> (8 * (j & 3))) & 0xffu;
                wf[nr][h] = __builtin_bit_cast(bf16x8_t, i4_to_bf16(*(const unsigned*)(rd4_ptr[kh][h] + nr * 2048), i4_group(sb, zb)));
              } else if constexpr (W4) {
                const unsigned sb = (sc4[f][nr][(2 * kh + h) >> 2] >> (8 * ((2 * kh + h) & 3))) & 0xffu;      // block 2 kh + h of the line
                wf[nr][h] = __builtin_bit_cast(bf16x8_t, mx4_to_bf16(*(const unsigned*)(rd4_ptr[kh][h] + nr * 2048), mx4_scale_f32(sb)));
              } else if constexpr (W8) {
                wf[nr][h] = __builtin_bit_cast(bf16x8_t, e4m3p2_to_bf16(*(const u32x2_t*)(rd8_ptr[kh][h] + nr * 2048), wsc[nr]));
              } else {
                wf[nr][h] = *(const bf16x8_t*)(rd_ptr[h] + nr * 2048);
              }
            }
          }
#pragma unroll
          for (int j = 0; j < XB; ++j) xf[j][h] = *(const bf16x8_t*)(rd_ptr[h] + (NR + j) * 2048);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int nr = 0; nr < NR; ++nr)
#pragma unroll
            for (int j = 0; j < XB; ++j)
              if (m0 + j < MB) acc[nr][m0 + j < MB ? m0 + j : 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nr][h], xf[j][h], acc[nr][m0 + j < MB ? m0 + j : 0], 0, 0, 0);
      }
     }
    }
  }
  __syncthreads();          // every wave is done with its slab before the reduction reuses the space

  // wave mb (< MB) finishes activation block mb: v = fp32 tile column (lane & 15) = activation row, rows 4 (lane >> 4) + i = weight rows
  auto epilogue = [&](int bid, float (&v)[4]) {
    const int m = 16 * wid + r;
    if (p.glu_I) {   // lanes g = 0,1 hold gate rows 4g+i, their partners 32 lanes up the matching up rows
      float u[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) u[i] = __shfl(v[i], (lane + 32) & 63, 64);
      if (g < 2 && m < p.M) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = rbf(silu_f(rbf(v[i]))) * rbf(u[i]);
        *(u32x2_t*)(p.C + (size_t)m * p.ldc + bid * 8 + 4 * g) = u32x2_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
      }
      return;
    }
    const int n = bid * 16 + 4 * g;
    if (m >= p.M) return;
    const bool second = p.C2 != nullptr && n >= p.n_split;
    const int act = second ? p.act2 : p.act;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float y = v[i];
      if (p.bias) y += bf2f(p.bias[n + i]);
      if (act != TD_ACT_NONE) y = act_rt(act, rbf(y));
      if (p.gate) y = rbf(y) * bf2f(p.gate[n + i]);
      if (p.res) y = rbf(y) + bf2f(p.res[(size_t)m * p.ldr + n + i]);
      v[i] = y;
    }
    const u32x2_t o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
    if (second) *(u32x2_t*)(p.C2 + (size_t)m * p.ldc2 + (n - p.n_split)) = o;
    else *(u32x2_t*)(p.C + (size_t)m * p.ldc + n) = o;
  };
  // partial tile of (block column, nr, mb, k-part): 64 lanes x 16 bytes
  const __amdgpu_buffer_rsrc_t rsP = __builtin_amdgcn_make_buffer_rsrc((void*)(ws + SPLITK_HEADER_BYTES), 0, (unsigned)SPLITK_PART_BYTES, 0x00020000);
  auto part = [&](int nr, int mb, int part_k) -> unsigned {
    return (unsigned)((((blockIdx.x * NR + nr) * MB + mb) * KS + part_k) * 64 + lane) * 16u;
  };

#pragma unroll
  for (int nr = 0; nr < NR; ++nr) {
    if (nr) __syncthreads();
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
      *(f32x4_t*)&red[wid][(mb * 64 + lane) * 4] = acc[nr][mb];
    __syncthreads();
    const int bid = blockIdx.x * NR + nr;
    if (wid >= MB || bid >= nblk) continue;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < MW; ++w) {
      const f32x4_t t = *(const f32x4_t*)&red[w][(wid * 64 + lane) * 4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += t[i];
    }
    if (KS == 1) epilogue(bid, v);
    else __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{as_u32(v[0]), as_u32(v[1]), as_u32(v[2]), as_u32(v[3])}, rsP, part(nr, wid, ky), 0, 16);   // aux 16 = sc1
  }
  if (KS == 1) return;
  // ---- split K: publish, draw the ticket, the last arriver sums the parts in index order and finishes ------------------------
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned* cnt = (unsigned*)ws + blockIdx.x;
  if (tid == 0) ticket_lds = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (ticket_lds != (unsigned)(KS - 1)) return;
  if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every ticket drawn: ready for the next launch
  if (wid >= MB) return;
#pragma unroll
  for (int nr = 0; nr < NR; ++nr) {
    const int bid = blockIdx.x * NR + nr;
    if (bid >= nblk) continue;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < KS; ++k) {
      const u32x4_t t = __builtin_amdgcn_raw_buffer_load_b128(rsP, part(nr, wid, k), 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += as_f32(t[i]);
    }
    epilogue(bid, v);
  }
}

// one hand-off workspace per (device, stream): launches on one stream never overlap
int splitk_workspace(hipStream_t stream, char** out) {
  struct Entry { int dev; hipStream_t stream; char* ws; };
  static std::mutex mu;
  static std::vector<Entry> pool;
  int dev = 0;
  TD_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  for (auto& e : pool)
    if (e.dev == dev && e.stream == stream) { *out = e.ws; return 0; }
  char* w = nullptr;
  TD_CHECK_HIP(hipMalloc((void**)&w, SPLITK_HEADER_BYTES + SPLITK_PART_BYTES));
  TD_CHECK_HIP(hipMemsetAsync(w, 0, SPLITK_HEADER_BYTES, stream));      // on the launching stream (ordered before the kernel)
  pool.push_back(Entry{dev, stream, w});
  *out = w;
  return 0;
}

// The weight forms of the stream kernels, as far as the host's shape rules go
struct WeightForm { int chunk, step, bits; };      // weights per 16-byte chunk (dot form), per MFMA k-step, and bits per weight
constexpr WeightForm FORM_BF16{8, 64, 16}, FORM_W8{16, 128, 8}, FORM_W4{32, 256, 4}, FORM_I4{32, 256, 4};
template <int WF> constexpr WeightForm form_of() { return WF == WF_I4 ? FORM_I4 : WF == WF_W4 ? FORM_W4 : WF == WF_W8 ? FORM_W8 : FORM_BF16; }

template <int MB, int NR, bool DEEP, int WF>
int launch_one(const TdGemmParams& p, dim3 grid, char* ws, hipStream_t stream) {
  constexpr int lds = gemv_lds_bytes<MB, NR>();
  if (lds + 64 >= 64 * 1024) {  // dynamic + the static ticket word reach the default 64 KiB limit: raise it once per device
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    TD_CHECK_HIP(hipGetDevice(&dev));
    if (!((done.load(std::memory_order_acquire) >> (dev & 63)) & 1ull)) {
      TD_CHECK_HIP(hipFuncSetAttribute((const void*)td_gemv_mfma_kernel<MB, NR, DEEP, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      done.fetch_or(1ull << (dev & 63), std::memory_order_release);
    }
  }
  hipLaunchKernelGGL((td_gemv_mfma_kernel<MB, NR, DEEP, WF>), grid, dim3(MW * 64), lds, stream, p, ws);
  return 0;
}

template <int MB, int WF>
int launch_mfma(const TdGemmParams& p, hipStream_t stream) {
  const int nblk = p.glu_I ? p.glu_I / 8 : p.N / 16;
  const int steps = p.K / form_of<WF>().step;      // k-steps of the kernel (64 elements; W8: 128, W4: 256 -- one line of weight bytes)
  // two weight blocks per workgroup halve the x re-reads from L2; only where the grid still oversubscribes the chip
  if (MB > 1 && nblk >= 1024) {
    const dim3 grid((nblk + 1) / 2);
    return steps >= 4 * MW ? launch_one<MB, 2, true, WF>(p, grid, nullptr, stream) : launch_one<MB, 2, false, WF>(p, grid, nullptr, stream);
  }
  // few block columns: split K over workgroups too, as long as every wave of a workgroup keeps at least one step
  int ks = 1;
  if (nblk < SPLITK_MAX_WGS / 2) ks = std::max(1, std::min({8, SPLITK_MAX_WGS / nblk, steps / MW}));
  char* ws = nullptr;
  if (ks > 1) {
    if (int rc = splitk_workspace(stream, &ws)) return rc;
  }
  const dim3 grid(nblk, ks);
  return steps / ks >= 4 * MW ? launch_one<MB, 1, true, WF>(p, grid, ws, stream) : launch_one<MB, 1, false, WF>(p, grid, ws, stream);
}

template <int WF>
int launch_mfma_rows(const TdGemmParams& p, hipStream_t stream) {
  if (p.M <= 16) return launch_mfma<1, WF>(p, stream);
  if (p.M <= 32) return launch_mfma<2, WF>(p, stream);
  if (p.M <= 48) return launch_mfma<3, WF>(p, stream);
  return launch_mfma<4, WF>(p, stream);
}

// the dot-product form's launch for M <= 16 rows
template <int WF>
void launch_dot(const TdGemmParams& p, dim3 grid, hipStream_t stream) {
  const dim3 block(THREADS);
  if (p.M == 1) hipLaunchKernelGGL((td_gemv_bf16_kernel<1, WF>), grid, block, 0, stream, p);
  else if (p.M == 2) hipLaunchKernelGGL((td_gemv_bf16_kernel<2, WF>), grid, block, 0, stream, p);
  else if (p.M <= 4) hipLaunchKernelGGL((td_gemv_bf16_kernel<4, WF>), grid, block, 0, stream, p);
  else if (p.M <= 8) hipLaunchKernelGGL((td_gemv_bf16_kernel<8, WF>), grid, block, 0, stream, p);
  else hipLaunchKernelGGL((td_gemv_bf16_kernel<16, WF>), grid, block, 0, stream, p);
}

// Shapes the matrix-core form takes.  Its operands sit behind 32-bit buffer descriptors, a k-step is whole, and the epilogue stores 4 columns (8 bytes) at
// a time.  `gated_checked`: the caller has already put a gated problem (glu_I) through the gated argument check (N == glu_I, a multiple of 8, ldc % 4, lda % 8,
// no split), which is all a gated launch needs -- its blocks are 8 gate + 8 up rows, so N % 16 is NOT asked.  td_gemv_mfma_ok asks it all the same.
bool mfma_ok(const TdGemmParams& p, WeightForm f, bool gated_checked) {
  const long long w_rows = p.glu_I ? 2ll * p.glu_I : p.N;
  if (w_rows * p.K * f.bits / 8 >= 0xFFFFFF00ll || ((long long)(p.M - 1) * p.lda + p.K) * 2 >= 0xFFFFFF00ll) return false;
  if (p.K % f.step != 0) return false;
  if (p.glu_I && gated_checked) return true;
  return p.N % 16 == 0 && p.ldc % 4 == 0 && p.lda % 8 == 0 && (!p.C2 || (p.ldc2 % 4 == 0 && p.n_split % 4 == 0));
}

// The routing tail of all forms: more than 4 rows and a shape the matrix core takes -> MFMA form, else the dot form (the caller has refused more than
// 16 rows without the MFMA form, in its own words).  W4 draws the line at 2 rows: a 4-bit weight byte meets four times the bytes of x a bf16 weight byte
// meets, every activation row reads them from L2 again, and at 3 .. 4 rows the dot form measured SLOWER than the bf16 kernels on W^ on the 2B decoder shape
// (2.19 vs 2.01 ms per step of 4 sequences) and level with them on the 7B one (3.78 vs 3.80), while the matrix-core form at 8 sequences took 1.48 / 2.54 ms
// (tools/bench_qwen2_w4.py)
template <int WF>
int route(const TdGemmParams& p, bool mfma, hipStream_t stream) {
  constexpr int DOT_ROWS = (WF == WF_W4 || WF == WF_I4) ? 2 : 4;      // (I4 streams the same bytes per weight and unpacks with more VALU work per row)
  if (p.M > DOT_ROWS && mfma) {
    if (int rc = launch_mfma_rows<WF>(p, stream)) return rc;
  } else {
    launch_dot<WF>(p, dim3(p.glu_I ? p.glu_I / 2 : p.N / R), stream);
  }
  TD_CHECK_LAUNCH();
  return 0;
}

// td_gemv_launch for TdGemmParams::W8.  It checks the leading dimensions and the alignment of every pointer itself (the bf16 entry below checks lda and
// the alignment of x and W only): the C ABI's 8-bit entries come straight here
int gemv_w8_launch(const TdGemmParams& p, hipStream_t stream) {
  TD_CHECK_ARG(p.W8 && p.w8_scale && p.A && p.C, "td_gemv(w8): x, the 8-bit weights, their row scales and the output are required");
  TD_CHECK_ARG(p.M >= 1 && p.M <= 64, "td_gemv(w8): M=%d: the 8-bit weight stream takes 1 .. 64 rows (more rows read the bf16 weights through td_linear_bf16)", p.M);
  TD_CHECK_ARG(p.N > 0 && p.N % R == 0 && p.K > 0 && p.K % 16 == 0, "td_gemv(w8): N=%d must be a multiple of 4 and K=%d a multiple of 16 (one 16-byte chunk of weight bytes)", p.N, p.K);
  TD_CHECK_ARG(p.lda >= p.K && p.lda % 8 == 0 && p.ldc >= (p.C2 ? p.n_split : p.N), "td_gemv(w8): bad leading dimensions lda=%d ldc=%d", p.lda, p.ldc);
  TD_CHECK_ARG(((uintptr_t)p.A | (uintptr_t)p.W8) % 16 == 0 && (uintptr_t)p.w8_scale % 4 == 0 && (uintptr_t)p.C % 8 == 0 && (uintptr_t)p.C2 % 8 == 0,
               "td_gemv(w8): misaligned operands: x and the weight bytes must be 16-byte aligned, the outputs 8-byte, the scales 4-byte");
  if (p.C2) TD_CHECK_ARG(p.n_split > 0 && p.n_split < p.N && p.n_split % 4 == 0 && p.ldc2 >= p.N - p.n_split, "td_gemv(w8): bad split-output arguments");
  if (p.glu_I) {
    TD_CHECK_ARG(p.N == p.glu_I && p.glu_I % 8 == 0 && !p.bias && !p.gate && !p.res && !p.C2 && p.act == TD_ACT_NONE && p.ldc % 4 == 0,
                 "td_gemv(w8, glu): N must equal glu_I (multiple of 8), no bias / gate / residual / split");
  }
  const bool mfma = mfma_ok(p, FORM_W8, true);
  TD_CHECK_ARG(p.M <= 16 || mfma, "td_gemv(w8): more than 16 rows need the matrix-core form (K=%d %% 128, N=%d %% 16, ldc %% 4 == 0, operands under 4 GiB)", p.K, p.N);
  return route<WF_W8>(p, mfma, stream);
}

// td_gemv_launch for TdGemmParams::W4, with the same duties as the 8-bit one above: the C ABI's 4-bit entries come straight here
int gemv_w4_launch(const TdGemmParams& p, hipStream_t stream) {
  TD_CHECK_ARG(!p.W8, "td_gemv(w4): W8 and W4 are exclusive");
  TD_CHECK_ARG(p.W4 && p.w4_scale && p.A && p.C, "td_gemv(w4): x, the packed 4-bit weights, their block scales and the output are required");
  TD_CHECK_ARG(p.M >= 1 && p.M <= 64, "td_gemv(w4): M=%d: the 4-bit weight stream takes 1 .. 64 rows (more rows read the bf16 weights through td_linear_bf16)", p.M);
  TD_CHECK_ARG(p.N > 0 && p.N % R == 0 && p.K > 0 && p.K % 32 == 0, "td_gemv(w4): N=%d must be a multiple of 4 and K=%d a multiple of 32 (one MX block = one 16-byte chunk of a packed row)", p.N, p.K);
  TD_CHECK_ARG(p.lda >= p.K && p.lda % 8 == 0 && p.ldc >= (p.C2 ? p.n_split : p.N), "td_gemv(w4): bad leading dimensions lda=%d ldc=%d", p.lda, p.ldc);
  TD_CHECK_ARG(((uintptr_t)p.A | (uintptr_t)p.W4) % 16 == 0 && (uintptr_t)p.w4_scale % 8 == 0 && (uintptr_t)p.C % 8 == 0 && (uintptr_t)p.C2 % 8 == 0,
               "td_gemv(w4): misaligned operands: x and the packed weights must be 16-byte aligned, the outputs and the scale bytes 8-byte");
  if (p.C2) TD_CHECK_ARG(p.n_split > 0 && p.n_split < p.N && p.n_split % 4 == 0 && p.ldc2 >= p.N - p.n_split, "td_gemv(w4): bad split-output arguments");
  if (p.glu_I) {
    TD_CHECK_ARG(p.N == p.glu_I && p.glu_I % 8 == 0 && !p.bias && !p.gate && !p.res && !p.C2 && p.act == TD_ACT_NONE && p.ldc % 4 == 0,
                 "td_gemv(w4, glu): N must equal glu_I (multiple of 8), no bias / gate / residual / split");
  }
  const bool mfma = mfma_ok(p, FORM_W4, true);
  TD_CHECK_ARG(p.M <= 16 || mfma, "td_gemv(w4): more than 16 rows need the matrix-core form (K=%d %% 256, N=%d %% 16, ldc %% 4 == 0, operands under 4 GiB)", p.K, p.N);
  return route<WF_W4>(p, mfma, stream);
}

// td_gemv_launch for TdGemmParams::I4, with the same duties and the same refusals as the two above: the C ABI's grouped-int4 entries come straight here
int gemv_i4_launch(const TdGemmParams& p, hipStream_t stream) {
  TD_CHECK_ARG(!p.W8 && !p.W4, "td_gemv(i4): W8, W4 and I4 are exclusive");
  TD_CHECK_ARG(p.I4 && p.i4_scale && p.i4_zero && p.A && p.C, "td_gemv(i4): x, the packed int4 weights, their group scales and zeros and the output are required");
  TD_CHECK_ARG(p.i4_gshift >= 5 && p.i4_gshift <= 7, "td_gemv(i4): G=%d: the group sizes served are 32, 64 and 128", p.i4_gshift >= 0 && p.i4_gshift < 31 ? 1 << p.i4_gshift : -1);
  TD_CHECK_ARG(p.M >= 1 && p.M <= 64, "td_gemv(i4): M=%d: the int4 weight stream takes 1 .. 64 rows (more rows read the bf16 weights through td_linear_bf16)", p.M);
  TD_CHECK_ARG(p.N > 0 && p.N % R == 0 && p.K > 0 && p.K % 32 == 0 && p.K % (1 << p.i4_gshift) == 0,
               "td_gemv(i4): N=%d must be a multiple of 4 and K=%d a multiple of G=%d and of 32 (one 16-byte chunk of a packed row)", p.N, p.K, 1 << p.i4_gshift);
  TD_CHECK_ARG(p.lda >= p.K && p.lda % 8 == 0 && p.ldc >= (p.C2 ? p.n_split : p.N), "td_gemv(i4): bad leading dimensions lda=%d ldc=%d", p.lda, p.ldc);
  TD_CHECK_ARG(((uintptr_t)p.A | (uintptr_t)p.I4 | (uintptr_t)p.i4_scale) % 16 == 0 && (uintptr_t)p.i4_zero % 8 == 0 && (uintptr_t)p.C % 8 == 0 && (uintptr_t)p.C2 % 8 == 0,
               "td_gemv(i4): misaligned operands: x, the packed weights and the scales must be 16-byte aligned, the outputs and the zeros 8-byte");
  if (p.C2) TD_CHECK_ARG(p.n_split > 0 && p.n_split < p.N && p.n_split % 4 == 0 && p.ldc2 >= p.N - p.n_split, "td_gemv(i4): bad split-output arguments");
  if (p.glu_I) {
    TD_CHECK_ARG(p.N == p.glu_I && p.glu_I % 8 == 0 && !p.bias && !p.gate && !p.res && !p.C2 && p.act == TD_ACT_NONE && p.ldc % 4 == 0,
                 "td_gemv(i4, glu): N must equal glu_I (multiple of 8), no bias / gate / residual / split");
  }
  const bool mfma = mfma_ok(p, FORM_I4, true);
  TD_CHECK_ARG(p.M <= 16 || mfma, "td_gemv(i4): more than 16 rows need the matrix-core form (K=%d %% 256, N=%d %% 16, ldc %% 4 == 0, operands under 4 GiB)", p.K, p.N);
  return route<WF_I4>(p, mfma, stream);
}

}  // namespace

// shapes the grouped int4 weight stream takes (csrc/qwen2_engine.hip asks before it routes a Linear to its int4 copy)
bool td_gemv_i4_ok(const TdGemmParams& p) {
  if (p.i4_gshift < 5 || p.i4_gshift > 7 || p.K % (1 << p.i4_gshift) != 0) return false;
  if (p.M < 1 || p.M > 64 || p.N % R != 0 || p.K % FORM_I4.chunk != 0 || p.lda % 8 != 0) return false;
  if (p.glu_I && (p.N != p.glu_I || p.glu_I % 8 != 0 || p.ldc % 4 != 0)) return false;
  return p.M <= 16 || mfma_ok(p, FORM_I4, true);
}

// shapes the 4-bit weight stream takes (csrc/qwen2_engine.hip asks before it routes a Linear to its MXFP4 copy)
bool td_gemv_w4_ok(const TdGemmParams& p) {
  if (p.M < 1 || p.M > 64 || p.N % R != 0 || p.K % FORM_W4.chunk != 0 || p.lda % 8 != 0) return false;
  if (p.glu_I && (p.N != p.glu_I || p.glu_I % 8 != 0 || p.ldc % 4 != 0)) return false;
  return p.M <= 16 || mfma_ok(p, FORM_W4, true);
}

// shapes the 8-bit weight stream takes (csrc/qwen2_engine.hip asks before it routes a Linear to its e4m3 copy)
bool td_gemv_w8_ok(const TdGemmParams& p) {
  if (p.M < 1 || p.M > 64 || p.N % R != 0 || p.K % FORM_W8.chunk != 0 || p.lda % 8 != 0) return false;
  if (p.glu_I && (p.N != p.glu_I || p.glu_I % 8 != 0 || p.ldc % 4 != 0)) return false;
  return p.M <= 16 || mfma_ok(p, FORM_W8, true);
}

// shapes the matrix-core weight stream takes (td_gemm_launch asks before routing 16 < M <= 64 here)
bool td_gemv_mfma_ok(const TdGemmParams& p) { return mfma_ok(p, FORM_BF16, false); }

int td_gemv_launch(const TdGemmParams& p, hipStream_t stream) {
  TD_CHECK_ARG(td_act_valid(p.act) && td_act_valid(p.act2), "td_gemv: unknown activation code act=%d act2=%d", p.act, p.act2);
  if (p.I4) return gemv_i4_launch(p, stream);
  if (p.W4) return gemv_w4_launch(p, stream);
  if (p.W8) return gemv_w8_launch(p, stream);
  TD_CHECK_ARG(p.M >= 1 && p.M <= 64 && p.N % R == 0 && p.K % FORM_BF16.chunk == 0 && p.lda % 8 == 0, "td_gemv: needs M <= 64, N %% 4 == 0, K %% 8 == 0");
  TD_CHECK_ARG(((uintptr_t)p.A | (uintptr_t)p.W) % 16 == 0, "td_gemv: operands must be 16-byte aligned");
  if (p.glu_I) {
    TD_CHECK_ARG(p.N == p.glu_I && p.glu_I % 8 == 0 && !p.bias && !p.gate && !p.res && !p.C2 && p.act == TD_ACT_NONE && p.ldc % 4 == 0,
                 "td_gemv(glu): N must equal glu_I (multiple of 8), no bias / gate / residual / split");
  }
  const bool mfma = mfma_ok(p, FORM_BF16, true);
  if (p.glu_I) TD_CHECK_ARG(p.M <= 16 || mfma, "td_gemv(glu): more than 16 rows need K %% 64 == 0 and operands under 4 GiB");
  else TD_CHECK_ARG(p.M <= 16 || mfma, "td_gemv: more than 16 rows need the matrix-core form (K %% 64, N %% 16, ldc %% 4 == 0)");
  return route<WF_BF16>(p, mfma, stream);
}
