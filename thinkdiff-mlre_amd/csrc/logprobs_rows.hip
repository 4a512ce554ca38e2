// Logprobs of rows of bf16 logits: the chosen token's log-probability and rank and the n largest logits of each row, one launch, one workgroup
// per row, no sort (td_logprobs_rows_bf16; the semantics are stated in include/thinkdiff_hip.h).  The logits are the RAW ones, before edits,
// penalties and temperature.
//   pass 0   row maximum (16-bit order-preserving key of the bf16 logit, NaN -> -inf, as sampler.hip);
//   pass 1   sum of exp(x - m) as 2^-40 fixed-point masses in 64-bit integers (integer sums: any order of accumulation gives the same bits, so a
//            row's result does not depend on its row index or on the launch's row count), the count of keys >= the chosen token's key (its
//            rank), and the count histogram over the high key byte;
//   pass 2   the count histogram over the low key byte inside the bin where the running count from the top reaches n -> the boundary key tau,
//            the number of tokens above it (< n) and how many of the tokens tied at tau complete the n;
//   pass 3/4 the tokens above tau are gathered (fewer than n <= 20: one thread orders them); the ties are taken in INDEX order: each wave walks a
//            contiguous range of chunks, so a tie's rank is (ties of earlier waves) + (ties of the wave's earlier chunks) + (ties of lower lanes),
//            a wave prefix sum per 64 chunks.
// A row with n_top = 0 stops after pass 1; the final ln and the differences x - lse are taken in double by the threads that write the few outputs.
#include "td_common.h"
#include "td_kernels.h"
#include "sampler_common.h"
#include "../../include/thinkdiff_hip.h"

namespace {

using namespace td_sampler_detail;

constexpr unsigned K16_PINF = 0xff80u, K16_NINF = 0x007fu;

// larger logit <-> larger key; NaN sorts with -inf (sampler.hip's key)
__device__ __forceinline__ unsigned key16(unsigned b) {
  if ((b & 0x7fffu) > 0x7f80u) b = 0xff80u;                       // NaN -> -inf
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float unkey16(unsigned k) {
  const unsigned b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
  return __builtin_bit_cast(float, b << 16);
}
__device__ __forceinline__ void keys8(const u32x4_t v, unsigned (&k)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    k[2 * j] = key16(v[j] & 0xffffu);
    k[2 * j + 1] = key16(v[j] >> 16);
  }
}

struct Lds {
  unsigned cnt[NW][256];      // per-wave count histograms
  unsigned cbins[256];
  unsigned scr32[NW + 1];
  u64 scr64[NW + 1];
  unsigned red[NW];
  unsigned wties[NW];
  int bin;
  unsigned above;
  unsigned n_gt;
  unsigned gt_key[TD_MAX_LOGPROBS];
  int gt_idx[TD_MAX_LOGPROBS];
  int top[TD_MAX_LOGPROBS];
};

// sum the per-wave histograms into cbins, then: the bin, scanning from the top with `base` tokens already in front, in which the running count
// first reaches `target`; leaves {bin, count in front of it} in L (a crossing exists whenever base + the histogram's total >= target)
__device__ __forceinline__ void fold_and_cross(Lds& L, unsigned base, unsigned target) {
  const int t = threadIdx.x;
  if (t < 256) {
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) n += L.cnt[i][t];
    L.cbins[t] = n;
  }
  if (t == 0) { L.bin = 0; L.above = base; }
  __syncthreads();
  const unsigned mine = t < 256 ? L.cbins[255 - t] : 0u;
  unsigned tot;
  const unsigned front = base + block_exclusive_scan<unsigned>(mine, L.scr32, &tot);
  if (t < 256 && mine > 0 && front < target && front + mine >= target) {
    L.bin = 255 - t;
    L.above = front;
  }
  __syncthreads();
}

__global__ __launch_bounds__(NT) void td_logprobs_rows_kernel(const bf16_t* __restrict__ logits, long long ld, int vocab, const int* __restrict__ ids,
                                                              const int* __restrict__ n_top, int top_cap, float* __restrict__ lp_sampled,
                                                              int* __restrict__ rank, int* __restrict__ top_ids, float* __restrict__ top_lp) {
  __shared__ Lds L;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row = blockIdx.x;
  int want = n_top[row];
  if (want < 0) return;                                  // skipped: outputs untouched (the whole workgroup leaves)
  want = want > top_cap ? top_cap : want;
  want = want > vocab ? vocab : want;
  const u32x4_t* src = (const u32x4_t*)(logits + (size_t)row * ld);
  const int nchunk = vocab >> 3;
  const int id = ids[row];
  const bool id_ok = id >= 0 && id < vocab;
  const unsigned kid = id_ok ? key16((unsigned)logits[(size_t)row * ld + id]) : 0u;

  // ---- pass 0: row maximum --------------------------------------------------------------------------------------------
  unsigned kmax = 0;
  for (int c = tid; c < nchunk; c += NT) {
    unsigned k[8];
    keys8(src[c], k);
#pragma unroll
    for (int e = 0; e < 8; ++e) kmax = max(kmax, k[e]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
  if (lane == 0) L.red[w] = kmax;
  __syncthreads();
  kmax = L.red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) kmax = max(kmax, L.red[i]);
  __syncthreads();
  const bool has_pinf = kmax == K16_PINF, none_finite = kmax <= K16_NINF;
  const float xmax = unkey16(kmax);

  // ---- pass 1: the sum, the rank and the high-byte count histogram ---------------------------------------------------
  for (int i = tid; i < NW * 256; i += NT) (&L.cnt[0][0])[i] = 0u;
  __syncthreads();
  u64 my_sum = 0;
  unsigned my_ge = 0;
  for (int c = tid; c < nchunk; c += NT) {
    unsigned k[8];
    keys8(src[c], k);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (!has_pinf && !none_finite) my_sum += (u64)(__builtin_amdgcn_exp2f((unkey16(k[e]) - xmax) * 1.4426950408889634f) * 1099511627776.0f);
      my_ge += k[e] >= kid ? 1u : 0u;
      if (want > 0) atomicAdd(&L.cnt[w][k[e] >> 8], 1u);
    }
  }
  u64 S;
  block_exclusive_scan<u64>(my_sum, L.scr64, &S);
  unsigned ge;
  block_exclusive_scan<unsigned>(my_ge, L.scr32, &ge);
  // lse in double (the maximum's own mass is 2^40, so S >= 2^40 on a regular row)
  const double lse = (double)xmax + (log((double)(S ? S : 1ull)) - 40.0 * 0.69314718055994530942);
  auto lp_of = [&](unsigned k) -> float {
    if (none_finite) return -INFINITY;
    if (has_pinf) return k == K16_PINF ? 0.f : -INFINITY;
    if (k <= K16_NINF) return -INFINITY;
    return (float)((double)unkey16(k) - lse);
  };
  if (tid == 0) {
    lp_sampled[row] = id_ok ? lp_of(kid) : -INFINITY;
    rank[row] = id_ok ? (int)ge : 0;
  }
  if (tid < top_cap && tid >= want) {                    // unused columns
    top_ids[(size_t)row * top_cap + tid] = -1;
    top_lp[(size_t)row * top_cap + tid] = -INFINITY;
  }
  if (want == 0) return;

  // ---- the boundary key: two count levels ------------------------------------------------------------------------------------
  fold_and_cross(L, 0u, (unsigned)want);
  const unsigned b_hi = (unsigned)L.bin;
  const unsigned above_hi = L.above;
  __syncthreads();
  for (int i = tid; i < NW * 256; i += NT) (&L.cnt[0][0])[i] = 0u;
  __syncthreads();
  for (int c = tid; c < nchunk; c += NT) {
    unsigned k[8];
    keys8(src[c], k);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if ((k[e] >> 8) == b_hi) atomicAdd(&L.cnt[w][k[e] & 255u], 1u);
  }
  __syncthreads();
  fold_and_cross(L, above_hi, (unsigned)want);
  const unsigned tau = (b_hi << 8) | (unsigned)L.bin;
  const unsigned above = L.above;                        // tokens with key > tau: fewer than want
  const unsigned need = (unsigned)want - above;          // ties at tau that complete the set, lowest indices first (1 .. n_tau)
  if (tid == 0) L.n_gt = 0u;
  __syncthreads();

  // ---- gather: wave w walks chunks [w * cpw, (w + 1) * cpw), lane-interleaved, so index order is (wave, iteration, lane, element) ----
  const int cpw = (nchunk + NW - 1) / NW;
  const int c0 = w * cpw, c1 = min(nchunk, c0 + cpw);
  unsigned my_ties = 0;
  for (int c = c0 + lane; c < c1; c += 64) {
    unsigned k[8];
    keys8(src[c], k);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (k[e] == tau) ++my_ties;
      else if (k[e] > tau) {
        const unsigned p = atomicAdd(&L.n_gt, 1u);
        if (p < (unsigned)TD_MAX_LOGPROBS) { L.gt_key[p] = k[e]; L.gt_idx[p] = 8 * c + e; }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) my_ties += (unsigned)__shfl_xor((int)my_ties, o, 64);
  if (lane == 0) L.wties[w] = my_ties;
  __syncthreads();
  unsigned running = 0;                                  // ties in front of this wave's range
  for (int i = 0; i < w; ++i) running += L.wties[i];
  for (int cb = c0; cb < c1 && running < need; cb += 64) {      // (wave-uniform bounds: every lane takes part in the shuffles)
    const int c = cb + lane;
    unsigned k[8];
    unsigned n = 0;
    if (c < c1) {
      keys8(src[c], k);
#pragma unroll
      for (int e = 0; e < 8; ++e) n += k[e] == tau ? 1u : 0u;
    }
    unsigned inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)inc, o, 64);
      if (lane >= o) inc += up;
    }
    unsigned r = running + inc - n;                      // rank of this lane's first tie
    if (c < c1 && n > 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (k[e] == tau) {
          if (r < need) L.top[above + r] = 8 * c + e;
          ++r;
        }
      }
    }
    running += (unsigned)__shfl((int)inc, 63, 64);
  }
  __syncthreads();
  // the tokens above tau, ordered by (key descending, index ascending): fewer than 20, one thread
  if (tid == 0) {
    const int n = (int)min(L.n_gt, above);
    for (int i = 1; i < n; ++i) {
      const unsigned kk = L.gt_key[i];
      const int ii = L.gt_idx[i];
      int j = i - 1;
      while (j >= 0 && (L.gt_key[j] < kk || (L.gt_key[j] == kk && L.gt_idx[j] > ii))) {
        L.gt_key[j + 1] = L.gt_key[j];
        L.gt_idx[j + 1] = L.gt_idx[j];
        --j;
      }
      L.gt_key[j + 1] = kk;
      L.gt_idx[j + 1] = ii;
    }
    for (int i = 0; i < n; ++i) L.top[i] = L.gt_idx[i];
  }
  __syncthreads();
  if (tid < want) {
    const int t = L.top[tid];
    top_ids[(size_t)row * top_cap + tid] = t;
    top_lp[(size_t)row * top_cap + tid] = lp_of(key16((unsigned)logits[(size_t)row * ld + t]));
  }
}

}  // namespace

extern "C" int td_logprobs_rows_bf16(const void* logits, int64_t ld, int rows, int vocab, const int32_t* ids_dev, const int32_t* n_top_dev, int top_cap,
                                     float* lp_sampled, int32_t* rank, int32_t* top_ids, float* top_lp, void* stream) {
  TD_CHECK_ARG(logits && ids_dev && n_top_dev && lp_sampled && rank, "td_logprobs_rows_bf16: null pointer (logits %p, ids %p, n_top %p, lp_sampled %p, rank %p)",
               logits, (const void*)ids_dev, (const void*)n_top_dev, (void*)lp_sampled, (void*)rank);
  TD_CHECK_ARG(top_cap >= 0 && top_cap <= TD_MAX_LOGPROBS, "td_logprobs_rows_bf16: top_cap must be in 0..%d (got %d)", TD_MAX_LOGPROBS, top_cap);
  TD_CHECK_ARG(top_cap == 0 || (top_ids && top_lp), "td_logprobs_rows_bf16: top_cap %d with a null top_ids / top_lp", top_cap);
  TD_CHECK_ARG(rows > 0 && rows <= 65535 && vocab >= 8, "td_logprobs_rows_bf16: need 1..65535 rows and vocab >= 8 (got %d, %d)", rows, vocab);
  TD_CHECK_ARG(vocab % 8 == 0 && ld % 8 == 0 && ld >= vocab && ((uintptr_t)logits) % 16 == 0,
               "td_logprobs_rows_bf16: vocab and row stride must be multiples of 8 (stride >= vocab), logits 16-byte aligned");
  hipLaunchKernelGGL(td_logprobs_rows_kernel, dim3(rows), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)logits, (long long)ld, vocab, ids_dev, n_top_dev,
                     top_cap, lp_sampled, rank, top_ids, top_lp);
  TD_CHECK_LAUNCH();
  return 0;
}
