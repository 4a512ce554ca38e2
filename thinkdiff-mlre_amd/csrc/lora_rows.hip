// Row-indexed low-rank add: the UNMERGED LoRA form, every row of a step or a prefill under an adapter of its own, behind a base Linear that stays as it is.
//
// Definition (everything is tested against it).  For a Linear y = x W^T (+ b) and a row whose adapter has A [r, K], B [N, r] (bf16) and scale s (fp32;
// lora_alpha / r, or lora_alpha / sqrt(r) under use_rslora):
//
//   t_j = bf16_rne( sum_k x_k A_jk )                                 fp32 accumulation, any order; products are exact
//   y_n = bf16_rne( float(y_base_n) + s * sum_j float(t_j) B_nj )    fp32 accumulation; ONE rounding
//
//  * y_base is whatever the base launch left in the output: the bf16 Linear result, or h + W x where the Linear adds its residual (o_proj, down_proj).
//  * t is rounded to bf16 at peft's rounding point (the output of lora_A; [ext] vLLM's punica expand casts its buffer to bf16 there too), which also lets
//    both halves run on the matrix core.
//  * s multiplies the fp32 sum and is never folded into a bf16 operand (the rule td_lora_merge_bf16 follows).
//  * A row with adapter index -1 is not touched: its output bytes are not written.  Neither is a row whose adapter has no operand for the segment.
//  * A row whose adapter has B = 0 gets back the value it had (as a value: -0 + 0 is +0).
//  * No float atomics: K is split over waves into S slabs, S a function of K alone (min(32, ceil(K / 256)) equal runs of 32-wide steps), the slabs' partial
//    sums go to the caller's workspace and are added in slab order, so two runs give the same bits, and a row's bits do not depend on how many rows ride
//    with it.
//
// Two kernels, both on v_mfma_f32_16x16x32_bf16, both computing the TRANSPOSED product so that the x row of a result sits on the lane column (l & 15) and
// four consecutive outputs of it on the lane's four accumulator registers (one 16-byte fp32 / 8-byte bf16 access):
//   shrink  P[slab][seg][row][j] = sum_{k in slab} A_jk x_k     MFMA "A" operand = A rows (16 ranks x 32 k), "B" operand = x^T; one wave per
//                                                               (16-row tile, slab), all segments' t in one pass over x
//   expand  y[row][n] += s * sum_j B_nj t_j                     MFMA "A" operand = B rows (16 n x 32 ranks), "B" operand = t^T, which every wave builds
//                                                               from the slabs in order; block-diagonal over the segments
// A 16-row tile with mixed adapters loops over the adapters present in it and feeds ZEROS for the rows that do not match (selected, not multiplied: a
// non-matching row never reaches the matrix core).  A column of the transposed product then holds its own adapter's sums alone, so one accumulator set
// serves all adapters of the tile.  The host does not sort rows; row_adapter is read on the device, so a captured step stays valid when it changes.
// Up to 256 rows (a decode step, bound by the latency of a wave's chain of operand reads, not by bytes) the adapters of a call ride on grid.z instead: block
// z serves the rows of adapter z alone, so four adapters in a tile cost the latency of one; a row's arithmetic is the same either way.
//
// Operand layout ("packed", td_lora_rows_pack_bf16, once per adapter and Linear segment): Ap [r_pad, K] = lora_A.weight, then Bp [N, r_pad] = lora_B.weight,
// the rank zero-padded to r_pad = 16 ceil(rank / 16) as td_lora_pack_bf16 does: every fragment is one 16-byte contiguous read.
#include <cmath>

#include "td_kernels.h"
#include "../../include/thinkdiff_hip.h"

namespace {

constexpr int LR_MAX_ADAPTERS = TD_LORA_MAX_ADAPTERS;
constexpr int LR_MAX_SEGS = TD_LORA_ROWS_MAX_SEGS;
constexpr int LR_MAX_RANK = TD_LORA_ROWS_MAX_RANK;
constexpr int LR_MAX_SLABS = 32;
constexpr int LR_Z_SPLIT_ROWS = 256;     // up to this many rows (a decode step) the adapters of a call ride on grid.z instead of a loop inside the wave
constexpr int LR_EXPAND_COLS = 256;      // output columns of one expand workgroup: 4 waves x 4 tiles of 16

struct LoraRowsArgs {
  const bf16_t* x; long long ldx;
  const int* row_adapter;
  int rows, K, n_adapters, n_segs;
  int RP;                 // rank stride of the workspace: the largest r_pad of the call
  int S, slab_steps;      // slabs and 32-wide k-steps per slab
  int z_split;            // 1: block z serves adapter z alone (its rows' partials and outputs; other rows are left to their own blocks)
  const bf16_t* Ap[LR_MAX_ADAPTERS][LR_MAX_SEGS];     // null: the adapter does not touch the segment
  const bf16_t* Bp[LR_MAX_ADAPTERS][LR_MAX_SEGS];
  int r_pad[LR_MAX_ADAPTERS];
  float scale[LR_MAX_ADAPTERS];
  bf16_t* y[LR_MAX_SEGS]; long long ldy[LR_MAX_SEGS]; int width[LR_MAX_SEGS];
  int chunk0[LR_MAX_SEGS + 1];                        // expand: first workgroup column chunk of every segment
  float* part;            // [S][n_segs][rows16][RP] fp32
};

inline int pad16(int r) { return (r + 15) & ~15; }
// slabs of K: a function of K alone (the summation order of a row must not depend on the rows around it)
inline void slab_plan(int K, int* S, int* steps) {
  const int ksteps = K / 32;
  int s = (K + 255) / 256;
  if (s > LR_MAX_SLABS) s = LR_MAX_SLABS;
  const int per = (ksteps + s - 1) / s;
  *steps = per;
  *S = (ksteps + per - 1) / per;
}

// the adapter of the lane's row: -1 past the last row and for anything outside 0 .. n_adapters - 1
__device__ __forceinline__ int lane_adapter(const LoraRowsArgs& a, int row) {
  int v = -1;
  if (row < a.rows) {
    v = a.row_adapter[row];
    if (v < 0 || v >= a.n_adapters) v = -1;
  }
  return v;
}

}  // namespace

// one thread per packed element
__global__ void td_lora_rows_pack_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, int rank, int r_pad, int N, int K,
                                         bf16_t* __restrict__ packed) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nA = (long long)K * r_pad, nB = (long long)N * r_pad;
  if (i >= nA + nB) return;
  bf16_t v = 0;
  if (i < nA) {
    const int r = (int)(i / K);
    if (r < rank) v = A[i];                          // (rows [0, rank) of Ap are lora_A.weight as it is)
  } else {
    const long long j = i - nA;
    const int n = (int)(j / r_pad), r = (int)(j % r_pad);
    if (r < rank) v = B[(size_t)n * rank + r];
  }
  packed[i] = v;
}

// grid (row tiles, ceil(S / 4)), 4 waves: wave w of block (t, b) owns slab 4 b + w of row tile t
__global__ __launch_bounds__(256) void td_lora_rows_shrink_kernel(LoraRowsArgs a) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int slab = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (slab >= a.S) return;                           // (wave-uniform; the kernel has no barrier)
  const int row = blockIdx.x * 16 + c;
  const int my_a = lane_adapter(a, row);
  const bool serve = a.z_split ? my_a == (int)blockIdx.z : my_a >= 0;      // the rows this wave answers for
  if (__ballot(serve) == 0) return;                  // none in the tile: the expand skips it too
  const int ks0 = slab * a.slab_steps;
  const int ks1 = min(ks0 + a.slab_steps, a.K >> 5);
  const bf16_t* xrow = a.x + (size_t)(my_a >= 0 ? row : 0) * a.ldx + 8 * g;

  f32x4_t acc[LR_MAX_SEGS][LR_MAX_RANK / 16];
#pragma unroll
  for (int sg = 0; sg < LR_MAX_SEGS; ++sg)
#pragma unroll
    for (int jb = 0; jb < LR_MAX_RANK / 16; ++jb) acc[sg][jb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int ad = 0; ad < LR_MAX_ADAPTERS; ++ad) {
    if (ad >= a.n_adapters) break;
    if (a.z_split && ad != (int)blockIdx.z) continue;
    const bool mine = my_a == ad;
    if (__ballot(mine) == 0) continue;
    const int nb = a.r_pad[ad] >> 4;
    // lane (c, g) of rank block jb reads Ap[16 jb + c][32 ks + 8 g ..+8)
    const bf16_t* ap[LR_MAX_SEGS];
#pragma unroll
    for (int sg = 0; sg < LR_MAX_SEGS; ++sg) ap[sg] = sg < a.n_segs && a.Ap[ad][sg] ? a.Ap[ad][sg] + (size_t)c * a.K + 8 * g : nullptr;
    for (int ks = ks0; ks < ks1; ++ks) {
      bf16x8_t xf = {0, 0, 0, 0, 0, 0, 0, 0};
      if (mine) xf = *(const bf16x8_t*)(xrow + 32 * ks);
#pragma unroll
      for (int sg = 0; sg < LR_MAX_SEGS; ++sg) {
        if (!ap[sg]) continue;
#pragma unroll
        for (int jb = 0; jb < LR_MAX_RANK / 16; ++jb) {
          if (jb >= nb) break;
          const bf16x8_t af = *(const bf16x8_t*)(ap[sg] + (size_t)jb * 16 * a.K + 32 * ks);
          acc[sg][jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf, acc[sg][jb], 0, 0, 0);
        }
      }
    }
  }

  // accumulator register i of lane (c, g), block jb = the slab's sum for row c, rank 16 jb + 4 g + i
  const int rows16 = gridDim.x * 16;
#pragma unroll
  for (int sg = 0; sg < LR_MAX_SEGS; ++sg) {
    if (sg >= a.n_segs) break;
    float* p = a.part + (((size_t)slab * a.n_segs + sg) * rows16 + row) * a.RP + 4 * g;
#pragma unroll
    for (int jb = 0; jb < LR_MAX_RANK / 16; ++jb)
      if (16 * jb < a.RP && (serve || !a.z_split)) *(f32x4_t*)(p + 16 * jb) = acc[sg][jb];      // (z_split: another block owns the other rows)
  }
}

// grid (row tiles, column chunks of all segments), 4 waves: wave w owns columns [chunk * 256 + 64 w, + 64) of its segment
__global__ __launch_bounds__(256) void td_lora_rows_expand_kernel(LoraRowsArgs a) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  int sg = 0;
#pragma unroll
  for (int i = 1; i < LR_MAX_SEGS; ++i)
    if (i < a.n_segs && (int)blockIdx.y >= a.chunk0[i]) sg = i;
  const int width = a.width[sg];
  const int n0 = ((int)blockIdx.y - a.chunk0[sg]) * LR_EXPAND_COLS + (threadIdx.x >> 6) * 64;
  if (n0 >= width) return;                           // (wave-uniform; no barrier)
  const int row = blockIdx.x * 16 + c;
  const int my_a = lane_adapter(a, row);
  const bool serve = a.z_split ? my_a == (int)blockIdx.z : my_a >= 0;
  if (__ballot(serve) == 0) return;
  const int rows16 = gridDim.x * 16;

  // t of the lane's row, ranks [32 u + 8 g, + 8): the slabs in order, one rounding
  bf16x8_t tf[LR_MAX_RANK / 32];
#pragma unroll
  for (int u = 0; u < LR_MAX_RANK / 32; ++u) {
    tf[u] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
    const int j0 = 32 * u + 8 * g;
    if (serve && j0 < a.RP) {
      float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < a.S; ++s) {
        const float* p = a.part + (((size_t)s * a.n_segs + sg) * rows16 + row) * a.RP + j0;
        const f32x4_t lo = *(const f32x4_t*)p, hi = *(const f32x4_t*)(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { sum[i] += lo[i]; sum[4 + i] += hi[i]; }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) tf[u][i] = (short)f2bf(sum[i]);
    }
  }

  f32x4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float sc = 0.f;
  bool touched = false;
#pragma unroll
  for (int ad = 0; ad < LR_MAX_ADAPTERS; ++ad) {
    if (ad >= a.n_adapters) break;
    if (a.z_split && ad != (int)blockIdx.z) continue;
    const bool mine = my_a == ad;
    if (__ballot(mine) == 0) continue;
    const bf16_t* bp = nullptr;
#pragma unroll
    for (int i = 0; i < LR_MAX_SEGS; ++i)
      if (i == sg) bp = a.Bp[ad][i];
    if (!bp) continue;
    if (mine) { touched = true; sc = a.scale[ad]; }
    const int rp = a.r_pad[ad];
#pragma unroll
    for (int u = 0; u < LR_MAX_RANK / 32; ++u) {
      if (32 * u >= rp) break;
      const bool live = 32 * u + 8 * g < rp;         // r_pad % 32 == 16: the upper half of the k-step multiplies zeros
      const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
      const bf16x8_t t = mine ? tf[u] : zero;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + 16 * nt;
        if (n >= width) break;
        // lane (c, g) reads Bp[n + c][32 u + 8 g ..+8)
        const bf16x8_t bf = live ? *(const bf16x8_t*)(bp + (size_t)(n + c) * rp + 32 * u + 8 * g) : zero;
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, t, acc[nt], 0, 0, 0);
      }
    }
  }
  if (!touched) return;
  // accumulator register i of lane (c, g), tile nt = the update of row c, column n0 + 16 nt + 4 g + i
  bf16_t* yrow = a.y[sg] + (size_t)row * a.ldy[sg] + n0 + 4 * g;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    if (n0 + 16 * nt >= width) break;
    const u32x2_t base = *(const u32x2_t*)(yrow + 16 * nt);
    u32x2_t o;
    o[0] = pack_bf2(bf_lo(base[0]) + sc * acc[nt][0], bf_hi(base[0]) + sc * acc[nt][1]);
    o[1] = pack_bf2(bf_lo(base[1]) + sc * acc[nt][2], bf_hi(base[1]) + sc * acc[nt][3]);
    *(u32x2_t*)(yrow + 16 * nt) = o;
  }
}

extern "C" {

size_t td_lora_rows_packed_bytes(int rank, int N, int K) {
  if (rank < 1 || N < 1 || K < 1) return 0;
  return (size_t)((long long)N + K) * pad16(rank) * sizeof(bf16_t);
}

int td_lora_rows_pack_bf16(const void* A, const void* B, int rank, int N, int K, void* packed, void* stream) {
  TD_CHECK_ARG(A && B && packed, "td_lora_rows_pack_bf16: null argument");
  TD_CHECK_ARG(rank >= 1 && rank <= LR_MAX_RANK, "td_lora_rows_pack_bf16: rank=%d outside 1..%d", rank, LR_MAX_RANK);
  TD_CHECK_ARG(N > 0 && K > 0 && K % 64 == 0 && N % 16 == 0, "td_lora_rows_pack_bf16: N=%d must be a positive multiple of 16, K=%d of 64", N, K);
  TD_CHECK_ARG((uintptr_t)packed % 16 == 0, "td_lora_rows_pack_bf16: packed must be 16-byte aligned");
  const int rp = pad16(rank);
  TD_GRID_1D(blocks, ((long long)N + K) * rp, 256, "td_lora_rows_pack_bf16");
  hipLaunchKernelGGL(td_lora_rows_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)A, (const bf16_t*)B, rank, rp, N, K,
                     (bf16_t*)packed);
  TD_CHECK_LAUNCH();
  return TD_OK;
}

size_t td_lora_rows_workspace_bytes(int rows, int K, int n_segs, int max_rank) {
  if (rows < 1 || K < 64 || K % 64 != 0 || n_segs < 1 || n_segs > LR_MAX_SEGS || max_rank < 1 || max_rank > LR_MAX_RANK) return 0;
  int S, steps;
  slab_plan(K, &S, &steps);
  const long long rows16 = ((long long)rows + 15) / 16 * 16;
  return (size_t)S * n_segs * rows16 * pad16(max_rank) * sizeof(float);
}

int td_lora_rows_bf16(const void* x, int64_t ldx, int rows, int K, const int32_t* row_adapter, int n_adapters, const void* const* packed, const int* ranks,
                      const float* scales, int n_segs, void* const* y, const int64_t* ldy, const int* widths, void* ws, size_t ws_bytes, void* stream) {
  TD_CHECK_ARG(x, "td_lora_rows_bf16: null x");
  TD_CHECK_ARG(row_adapter, "td_lora_rows_bf16: null row_adapter");
  TD_CHECK_ARG(n_adapters >= 0 && n_adapters <= LR_MAX_ADAPTERS, "td_lora_rows_bf16: n_adapters=%d, one call takes at most %d", n_adapters, LR_MAX_ADAPTERS);
  TD_CHECK_ARG(n_segs >= 1 && n_segs <= LR_MAX_SEGS, "td_lora_rows_bf16: n_segs=%d outside 1..%d", n_segs, LR_MAX_SEGS);
  TD_CHECK_ARG(n_adapters == 0 || (packed && ranks && scales), "td_lora_rows_bf16: null packed / ranks / scales with %d adapters", n_adapters);
  TD_CHECK_ARG(y && ldy && widths, "td_lora_rows_bf16: null y / ldy / widths");
  TD_CHECK_ARG(rows >= 1 && rows < (1 << 24), "td_lora_rows_bf16: rows=%d outside 1..2^24", rows);
  TD_CHECK_ARG(K >= 64 && K % 64 == 0, "td_lora_rows_bf16: K=%d must be a positive multiple of 64", K);
  TD_CHECK_ARG(ldx >= K && ldx % 8 == 0 && (uintptr_t)x % 16 == 0, "td_lora_rows_bf16: ldx=%lld must be at least K=%d and a multiple of 8, x 16-byte aligned", (long long)ldx, K);
  LoraRowsArgs a;
  a.x = (const bf16_t*)x; a.ldx = ldx; a.row_adapter = row_adapter; a.rows = rows; a.K = K; a.n_adapters = n_adapters; a.n_segs = n_segs;
  a.chunk0[0] = 0;
  for (int s = 0; s < LR_MAX_SEGS; ++s) {
    a.y[s] = nullptr; a.ldy[s] = 0; a.width[s] = 0;
    if (s >= n_segs) { a.chunk0[s + 1] = a.chunk0[s]; continue; }
    TD_CHECK_ARG(y[s], "td_lora_rows_bf16: segment %d: null y", s);
    TD_CHECK_ARG(widths[s] >= 16 && widths[s] % 16 == 0, "td_lora_rows_bf16: segment %d: width=%d must be a positive multiple of 16", s, widths[s]);
    TD_CHECK_ARG(ldy[s] >= widths[s] && ldy[s] % 4 == 0 && (uintptr_t)y[s] % 8 == 0,
                 "td_lora_rows_bf16: segment %d: ldy=%lld must be at least width=%d and a multiple of 4, y 8-byte aligned", s, (long long)ldy[s], widths[s]);
    a.y[s] = (bf16_t*)y[s]; a.ldy[s] = ldy[s]; a.width[s] = widths[s];
    a.chunk0[s + 1] = a.chunk0[s] + (widths[s] + LR_EXPAND_COLS - 1) / LR_EXPAND_COLS;
  }
  int rp_max = 0;
  for (int i = 0; i < LR_MAX_ADAPTERS; ++i) {
    a.r_pad[i] = 0; a.scale[i] = 0.f;
    for (int s = 0; s < LR_MAX_SEGS; ++s) a.Ap[i][s] = a.Bp[i][s] = nullptr;
    if (i >= n_adapters) continue;
    bool any = false;
    for (int s = 0; s < n_segs; ++s) any = any || packed[(size_t)i * n_segs + s];
    if (!any) continue;                              // the adapter does not touch this Linear: its rank and scale are not looked at
    TD_CHECK_ARG(ranks[i] >= 1 && ranks[i] <= LR_MAX_RANK, "td_lora_rows_bf16: adapter %d: rank=%d outside 1..%d", i, ranks[i], LR_MAX_RANK);
    TD_CHECK_ARG(std::isfinite(scales[i]), "td_lora_rows_bf16: adapter %d: scale is not finite", i);
    a.r_pad[i] = pad16(ranks[i]); a.scale[i] = scales[i];
    rp_max = a.r_pad[i] > rp_max ? a.r_pad[i] : rp_max;
    for (int s = 0; s < n_segs; ++s) {
      const bf16_t* p = (const bf16_t*)packed[(size_t)i * n_segs + s];
      if (!p) continue;
      TD_CHECK_ARG((uintptr_t)p % 16 == 0, "td_lora_rows_bf16: adapter %d, segment %d: packed operands must be 16-byte aligned", i, s);
      a.Ap[i][s] = p;
      a.Bp[i][s] = p + (size_t)a.r_pad[i] * K;
    }
  }
  if (rp_max == 0) return TD_OK;                     // no adapter touches this Linear: nothing is launched, nothing written
  slab_plan(K, &a.S, &a.slab_steps);
  a.RP = rp_max;
  const long long tiles = ((long long)rows + 15) / 16;
  const size_t need = (size_t)a.S * n_segs * tiles * 16 * rp_max * sizeof(float);
  TD_CHECK_ARG(ws && (uintptr_t)ws % 16 == 0, "td_lora_rows_bf16: the workspace ws is required, 16-byte aligned");
  TD_CHECK_ARG(ws_bytes >= need, "td_lora_rows_bf16: ws_bytes=%zu, but %d rows x %d segments x rank %d in %d slabs of K=%d need %zu (td_lora_rows_workspace_bytes)", ws_bytes,
               rows, n_segs, rp_max, a.S, K, need);
  a.part = (float*)ws;
  a.z_split = rows <= LR_Z_SPLIT_ROWS && n_adapters > 1 ? 1 : 0;
  const unsigned gz = a.z_split ? (unsigned)n_adapters : 1u;
  hipLaunchKernelGGL(td_lora_rows_shrink_kernel, dim3((unsigned)tiles, (unsigned)((a.S + 3) / 4), gz), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(td_lora_rows_expand_kernel, dim3((unsigned)tiles, (unsigned)a.chunk0[n_segs], gz), dim3(256), 0, (hipStream_t)stream, a);
  TD_CHECK_LAUNCH();
  return TD_OK;
}

}  // extern "C"
