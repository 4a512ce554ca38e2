// Per-request sampling over rows of bf16 logits: repetition / presence / frequency penalties, top-k, top-p and min-p, every value per row,
// one launch, one workgroup per row, no sort (td_sample_rows_bf16; the semantics are stated in include/thinkdiff_hip.h).
//
// sampler.hip finds the nucleus boundary by a two-level radix select on the 16-bit key of a bf16 logit.  A penalised logit is an fp32 value, so
// the key here is the order-preserving 32-bit key of the fp32 value z; an unpenalised token's key has its low 16 bits clear.  The kept set of each
// filter is a prefix of the tokens in descending key order, so the intersection is the shortest prefix, described by (tau, keep): every token with
// key > tau and the first `keep` tokens (in the kernel's walk order) with key == tau.
//   pass 0   row maximum of z (penalties applied: a penalised former maximum is not the maximum);
//   select   a radix select over 8 key bits per level, each level one pass over the row building mass, count and "low bits set" histograms of
//            the tokens inside the prefix chosen so far.  A level's bin is final as soon as no token in it has a key bit set below the level:
//            after TWO levels unless a penalised token shares the boundary bin (then a third and a fourth level order it exactly).
//            top-k selects by count and yields the top-k mass Zk; top-p then selects by mass against top_p x Zk, reusing the first level's
//            histograms.  A filter that is off costs no pass;
//   min-p    a key threshold, key(zmax + T ln(min_p)): no pass;
//   draw     sampler.hip's pass 3 on (tau, keep): masses of the kept tokens, a prefix sum in thread order, one uniform r, one walk to locate it.
// Masses are 2^-40 fixed point as in sampler.hip, so sums do not depend on the order of the LDS atomics and (seed, offset, stream) fixes the
// token; with no history and every filter off the arithmetic is sampler.hip's and so are the ids.
// History: per slot a bitmap of the tokens with history (one byte per 16-byte chunk of logits, read beside it) and a uint16 count per token,
// read only for flagged tokens.  Row reads: 2 (greedy), 4 (top-p, as sampler.hip), 4 (top-k alone), 5 (top-k + top-p), +2 per select whose
// boundary bin holds a penalised token.
// Logit edits (td_sample_rows_edit_bf16; the kernel's EDIT form, a template parameter: the form without edits is the code above unchanged): per edit
// slot a ban bitmap and a bias bitmap (one byte of each per chunk, read beside the logits as the history byte is: both unconditionally, so that an
// edited chunk costs no second, dependent trip to memory) and a table of at most TD_MAX_LOGIT_BIAS (token, fp32 value) pairs sorted by token,
// which the workgroup stages in LDS once and searches only for biased tokens.  A banned token's key is -inf's; a biased token's key is the fp32 key
// of float(x) + b, ordered exactly by the third and fourth select levels like a penalised token's.
#include <algorithm>
#include "td_common.h"
#include "td_kernels.h"
#include "sampler_common.h"
#include "../../include/thinkdiff_hip.h"

struct td_sampler {
  int n_slots, vocab;
  long long bm_stride;      // bytes per slot of a bitmap: vocab / 8 rounded up to 4
  uint8_t* prompt;          // [n_slots, bm_stride] bit t: token t is in the prompt
  uint8_t* seen;            // [n_slots, bm_stride] bit t: token t is in the prompt or was generated (count > 0)
  uint16_t* counts;         // [n_slots, vocab]
};

struct td_logit_edits {
  int n_slots, vocab;
  long long bm_stride;      // bytes per slot of a bitmap: vocab / 8 rounded up to 4
  uint8_t* ban;             // [n_slots, bm_stride] bit t: token t is banned
  uint8_t* bias;            // [n_slots, bm_stride] bit t: token t has an entry in the slot's table
  int* tok;                 // [n_slots, TD_MAX_LOGIT_BIAS] the biased tokens, ascending
  float* val;               // [n_slots, TD_MAX_LOGIT_BIAS]
  int* n;                   // [n_slots] table entries in use
};

namespace {

using namespace td_sampler_detail;
constexpr unsigned KEY_PINF = 0xff800000u, KEY_NINF = 0x007f0000u;

// larger value <-> larger key; a value whose low 16 mantissa bits are clear (a bf16) has a key whose low 16 bits are clear, either sign
__device__ __forceinline__ unsigned key32(unsigned b) {
  if ((b & 0x7fffffffu) > 0x7f800000u) b = 0xff800000u;            // NaN -> -inf
  return (b & 0x80000000u) ? (0x7fff0000u - (b & 0x7fffffffu)) : (b | 0x80000000u);
}
__device__ __forceinline__ float unkey32(unsigned k) {
  return as_f32((k & 0x80000000u) ? (k & 0x7fffffffu) : (0x80000000u | (0x7fff0000u - k)));
}

struct Row {
  const u32x4_t* src;         // the row's logits, 8 per chunk
  const uint8_t* seen;        // the slot's history bitmap, one byte per chunk; NULL: no penalty applies
  const uint16_t* counts;
  float rep, pres, freq;
  float zmax, c2;             // set after pass 0
  // the EDIT form only: the edit slot's two bitmaps (eban NULL: no edits) and its sorted bias table (in LDS)
  const uint8_t* eban;
  const uint8_t* ebias;
  const TD_LDS int* btok;
  const TD_LDS float* bval;
  int nbias;
};

// the bias of token t: a binary search of the slot's sorted table (0 if the table does not hold it)
__device__ __forceinline__ float bias_of(const Row& R, int t) {
  int lo = 0, hi = R.nbias;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (R.btok[mid] < t) lo = mid + 1; else hi = mid;
  }
  return (lo < R.nbias && R.btok[lo] == t) ? R.bval[lo] : 0.f;
}

// keys of the 8 tokens of chunk c: edits (EDIT form), then penalties
template <bool EDIT>
__device__ __forceinline__ void keys8(const Row& R, int c, unsigned (&k)[8]) {
  const u32x4_t v = R.src[c];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    k[2 * j] = key32(v[j] << 16);
    k[2 * j + 1] = key32(v[j] & 0xffff0000u);
  }
  unsigned banned = 0u;
  if (EDIT && R.eban) {
    banned = R.eban[c];
    const unsigned biased = R.ebias[c] & ~banned;                   // a banned token stays banned whatever its bias
    if (banned | biased) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if ((banned >> e) & 1u) k[e] = KEY_NINF;
        else if ((biased >> e) & 1u) k[e] = key32(as_u32(unkey32(k[e]) + bias_of(R, 8 * c + e)));      // (inf - inf = NaN -> -inf)
      }
    }
  }
  if (R.seen) {
    const unsigned f = R.seen[c] & ~banned;                         // (-inf stays -inf under every penalty: nothing to do for a banned token)
    if (f) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if ((f >> e) & 1u) {
          const float cn = (float)R.counts[8 * c + e];
          float z = unkey32(k[e]);                                  // (NaN already -inf)
          z = z > 0.f ? z / R.rep : z * R.rep;
          z -= R.freq * cn;
          z -= cn > 0.f ? R.pres : 0.f;
          k[e] = key32(as_u32(z));
        }
      }
    }
  }
}
// un-normalised probability of a key as 2^-40 fixed point: exp((z - zmax) / T) in [0, 1]
__device__ __forceinline__ u64 mass_of(const Row& R, unsigned k) {
  const float e = __builtin_amdgcn_exp2f((unkey32(k) - R.zmax) * R.c2);
  return (u64)(e * 1099511627776.0f);
}

struct Lds {
  u64 hist[NW][256];          // per-wave mass histograms (32 KiB)
  unsigned cnt[NW][256];      // per-wave count histograms (16 KiB)
  u64 bins[256], bins1[256];  // the current level's masses; the first level's, kept for the second select
  unsigned cbins[256], cbins1[256];
  unsigned xbins[256];        // tokens of the bin with a key bit set below the level (penalised tokens only: plain LDS atomics)
  u64 scr64[NW + 1];
  unsigned scr32[NW + 1];
  unsigned red[NW];
  int bin;
  u64 above_m, above_c;
  int pick;
};

struct Cut {                  // a prefix of the descending key order
  unsigned tau;               // boundary key
  unsigned n_tau;             // tokens with key == tau
  u64 above_m, above_c;       // mass and count of the tokens with key > tau
};

// One histogram level: tokens with (key >> (shift + 8)) == prefix (all tokens at shift 24) fall into bin (key >> shift) & 255.
template <bool EDIT>
__device__ __forceinline__ void hist_level(const Row& R, Lds& L, int nchunk, int shift, unsigned prefix, bool count) {
  const int tid = threadIdx.x, w = tid >> 6;
  for (int i = tid; i < NW * 256; i += NT) { (&L.hist[0][0])[i] = 0ull; (&L.cnt[0][0])[i] = 0u; }
  if (tid < 256) L.xbins[tid] = 0u;
  __syncthreads();
  const unsigned low = (1u << shift) - 1u;
  for (int c = tid; c < nchunk; c += NT) {
    unsigned k[8];
    keys8<EDIT>(R, c, k);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (shift == 24 || (k[e] >> (shift + 8)) == prefix) {
        const unsigned b = (k[e] >> shift) & 255u;
        const u64 m = mass_of(R, k[e]);
        if (m) atomicAdd(&L.hist[w][b], m);
        if (count) atomicAdd(&L.cnt[w][b], 1u);
        if (shift < 24 && (k[e] & low)) atomicAdd(&L.xbins[b], 1u);
      }
    }
  }
  __syncthreads();
  if (tid < 256) {
    u64 s = 0;
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { s += L.hist[i][tid]; n += L.cnt[i][tid]; }
    L.bins[tid] = s;
    L.cbins[tid] = n;
  }
  __syncthreads();
}

// Among the 256 bins of the current level, scanning from the top with (base_m, base_c) already in front: the bin in which the running mass
// (by_count: the running count) first reaches `target`.  Leaves {bin, mass in front, count in front} in L; the defaults stand if none matches.
__device__ __forceinline__ void find_crossing(Lds& L, bool by_count, u64 base_m, u64 base_c, u64 target) {
  const int t = threadIdx.x;
  if (t == 0) { L.bin = 255; L.above_m = base_m; L.above_c = base_c; }
  const u64 mine_m = t < 256 ? L.bins[255 - t] : 0ull;
  const u64 mine_c = t < 256 ? (u64)L.cbins[255 - t] : 0ull;
  u64 tot;
  const u64 front_m = base_m + block_exclusive_scan<u64>(mine_m, L.scr64, &tot);
  const u64 front_c = base_c + block_exclusive_scan<u64>(mine_c, L.scr64, &tot);
  const u64 mine = by_count ? mine_c : mine_m, front = by_count ? front_c : front_m;
  if (t < 256 && mine > 0 && front < target && front + mine >= target) {
    L.bin = 255 - t;
    L.above_m = front_m;
    L.above_c = front_c;
  }
  __syncthreads();
}

// Radix select: the key at which the running mass (count) from the top reaches target.  have_l1: the first level's histograms are in bins1 /
// cbins1 (built with counts iff count_l1); otherwise they are built and left there.
template <bool EDIT>
__device__ __forceinline__ Cut select(const Row& R, Lds& L, int nchunk, bool by_count, u64 target, bool have_l1, bool count_l1) {
  const int tid = threadIdx.x;
  unsigned prefix = 0;
  Cut cut = {0u, 0u, 0ull, 0ull};
  int shift = 24;
  for (;; shift -= 8) {
    if (shift == 24 && have_l1) {
      if (tid < 256) { L.bins[tid] = L.bins1[tid]; L.cbins[tid] = L.cbins1[tid]; }
      __syncthreads();
    } else {
      hist_level<EDIT>(R, L, nchunk, shift, prefix, shift < 24 || count_l1);
      if (shift == 24) {
        if (tid < 256) { L.bins1[tid] = L.bins[tid]; L.cbins1[tid] = L.cbins[tid]; }
        __syncthreads();
      }
    }
    find_crossing(L, by_count, cut.above_m, cut.above_c, target);
    const int b = L.bin;
    cut.above_m = L.above_m;
    cut.above_c = L.above_c;
    cut.n_tau = L.cbins[b];
    const unsigned xb = shift < 24 ? L.xbins[b] : 1u;
    __syncthreads();
    prefix = (prefix << 8) | (unsigned)b;
    if (shift == 0 || xb == 0u) break;      // every token of the bin has the same key
  }
  cut.tau = prefix << shift;
  return cut;
}

// the edit state as the kernel sees it (EDIT form; by value in the kernel arguments)
struct EditView {
  const uint8_t* ban;         // [n_slots, bm_stride]
  const uint8_t* bias;        // [n_slots, bm_stride]
  const int* tok;             // [n_slots, TD_MAX_LOGIT_BIAS] sorted
  const float* val;           // [n_slots, TD_MAX_LOGIT_BIAS]
  const int* n;               // [n_slots] entries in use
  const int* row_slot;        // [rows] the edit slot of each row, outside [0, n_slots): none
  long long bm_stride;
  int n_slots;
};

template <bool EDIT>
__global__ __launch_bounds__(NT) void td_sample_rows_kernel(const bf16_t* __restrict__ logits, long long ld, int vocab,
                                                            const TdSampleRow* __restrict__ params, const long long* __restrict__ offsets,
                                                            uint8_t* seen, uint16_t* counts, long long bm_stride, int n_slots, int update_state,
                                                            int* __restrict__ out, const EditView E) {
  __shared__ Lds L;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row = blockIdx.x;
  const int nchunk = vocab >> 3;                     // 8 logits per 16-byte chunk
  const TdSampleRow P = params[row];
  const float temperature = P.temperature;
  float top_p = P.top_p;
  if (!(top_p <= 1.0f)) top_p = 1.0f;                // above 1 or NaN
  float min_p = P.min_p;
  if (!(min_p > 0.f)) min_p = 0.f;
  if (min_p > 1.0f) min_p = 1.0f;
  const bool fin_rep = P.repetition_penalty > 0.f && P.repetition_penalty < INFINITY;
  const float rep = fin_rep ? P.repetition_penalty : 1.0f;
  const float pres = fabsf(P.presence_penalty) < INFINITY ? P.presence_penalty : 0.f;
  const float freq = fabsf(P.frequency_penalty) < INFINITY ? P.frequency_penalty : 0.f;
  const bool has_slot = seen != nullptr && P.slot >= 0 && P.slot < n_slots;
  const bool penalised = has_slot && (rep != 1.0f || pres != 0.f || freq != 0.f);
  const bool use_k = P.top_k > 0 && P.top_k < vocab;

  Row R;
  R.src = (const u32x4_t*)(logits + (size_t)row * ld);
  R.seen = penalised ? seen + (size_t)P.slot * bm_stride : nullptr;
  R.counts = penalised ? counts + (size_t)P.slot * vocab : nullptr;
  R.rep = rep; R.pres = pres; R.freq = freq;
  R.zmax = 0.f; R.c2 = 0.f;
  R.eban = nullptr; R.ebias = nullptr; R.btok = nullptr; R.bval = nullptr; R.nbias = 0;
  static_assert(NT >= TD_MAX_LOGIT_BIAS, "one bias-table entry per thread");
  __shared__ int s_btok[EDIT ? TD_MAX_LOGIT_BIAS : 1];
  __shared__ float s_bval[EDIT ? TD_MAX_LOGIT_BIAS : 1];
  if (EDIT) {
    const int es = E.row_slot[row];
    if (es >= 0 && es < E.n_slots) {                     // (the same for every thread of the workgroup)
      R.eban = E.ban + (size_t)es * E.bm_stride;
      R.ebias = E.bias + (size_t)es * E.bm_stride;
      R.nbias = min(max(E.n[es], 0), TD_MAX_LOGIT_BIAS);
      if (tid < R.nbias) {                               // NT == TD_MAX_LOGIT_BIAS: one entry per thread
        s_btok[tid] = E.tok[(size_t)es * TD_MAX_LOGIT_BIAS + tid];
        s_bval[tid] = E.val[(size_t)es * TD_MAX_LOGIT_BIAS + tid];
      }
      R.btok = (const TD_LDS int*)s_btok;
      R.bval = (const TD_LDS float*)s_bval;
      __syncthreads();
    }
  }

  // the thread that writes the token also records it in the slot's history
  auto emit = [&](int tok) {
    tok = (unsigned)tok < (unsigned)vocab ? tok : 0;
    out[row] = tok;
    if (update_state && has_slot) {
      uint16_t* cp = counts + (size_t)P.slot * vocab + tok;
      const unsigned cv = *cp;
      if (cv < 65535u) *cp = (uint16_t)(cv + 1u);
      seen[(size_t)P.slot * bm_stride + (tok >> 3)] |= (uint8_t)(1u << (tok & 7));
    }
  };

  // ---- pass 0: row maximum (as a key) ------------------------------------------------------------------------------
  unsigned kmax = 0;
  for (int c = tid; c < nchunk; c += NT) {
    unsigned k[8];
    keys8<EDIT>(R, c, k);
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

  // greedy, or a +inf value (it has all the mass): the first index holding the maximum
  if (!(temperature > 0.f) || kmax == KEY_PINF) {
    unsigned best = 0xffffffffu;
    for (int c = tid; c < nchunk; c += NT) {
      unsigned k[8];
      keys8<EDIT>(R, c, k);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k[e] == kmax) best = min(best, (unsigned)(8 * c + e));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 64));
    if (lane == 0) L.red[w] = best;
    __syncthreads();
    if (tid == 0) {
      unsigned b = L.red[0];
      for (int i = 1; i < NW; ++i) b = min(b, L.red[i]);
      emit((int)b);
    }
    return;
  }
  if (kmax <= KEY_NINF) {                              // no finite value in the row: nothing to weigh
    if (tid == 0) emit(0);
    return;
  }
  R.zmax = unkey32(kmax);
  R.c2 = 1.4426950408889634f / temperature;

  // ---- the cut (tau, keep): shortest of the top-k, top-p and min-p prefixes ---------------------------------------------
  unsigned tau = 0u;
  u64 keep = ~0ull;
  bool have_l1 = false;
  u64 Zk = 0;
  if (use_k) {
    const Cut ck = select<EDIT>(R, L, nchunk, true, (u64)P.top_k, false, true);
    have_l1 = true;
    u64 kk = (u64)P.top_k - ck.above_c;
    kk = kk < 1 ? 1 : (kk > ck.n_tau ? ck.n_tau : kk);
    tau = ck.tau;
    keep = kk;
    Zk = ck.above_m + kk * mass_of(R, ck.tau);
  }
  if (top_p < 1.0f) {
    if (!use_k) {                                      // Z: the whole row's mass, from the first level
      hist_level<EDIT>(R, L, nchunk, 24, 0u, false);
      if (tid < 256) { L.bins1[tid] = L.bins[tid]; L.cbins1[tid] = L.cbins[tid]; }
      __syncthreads();
      have_l1 = true;
      block_exclusive_scan<u64>(tid < 256 ? L.bins[tid] : 0ull, L.scr64, &Zk);
    }
    u64 target = top_p > 0.f ? (u64)((double)top_p * (double)Zk) : 1ull;
    target = target < 1ull ? 1ull : (target > Zk ? Zk : target);
    const Cut cp = select<EDIT>(R, L, nchunk, false, target, have_l1, use_k);
    u64 m_tau = mass_of(R, cp.tau);                    // > 0 when the crossing bin holds mass
    m_tau = m_tau ? m_tau : 1ull;
    u64 kp = (target - cp.above_m + m_tau - 1) / m_tau;      // ties kept: the j-th is kept iff above + j * m_tau < target
    kp = kp < 1 ? 1 : (kp > cp.n_tau ? cp.n_tau : kp);
    if (!use_k || cp.tau > tau) { tau = cp.tau; keep = kp; }
    else if (cp.tau == tau) keep = kp < keep ? kp : keep;
  }
  if (min_p > 0.f) {
    const unsigned kthr = key32(as_u32(R.zmax + temperature * logf(min_p)));
    if (kthr > tau) { tau = kthr > kmax ? kmax : kthr; keep = ~0ull; }
  }

  // ---- draw r in [0, kept mass) and locate it (token order: thread-major, any fixed order gives the same law) ---------
  unsigned my_ties = 0;
  u64 my_gt = 0;
  for (int c = tid; c < nchunk; c += NT) {
    unsigned k[8];
    keys8<EDIT>(R, c, k);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (k[e] > tau) my_gt += mass_of(R, k[e]); else if (k[e] == tau) ++my_ties;
    }
  }
  u64 m_tau = mass_of(R, tau);
  m_tau = m_tau ? m_tau : 1ull;
  unsigned tie_total;
  const unsigned tie_off = block_exclusive_scan<unsigned>(my_ties, L.scr32, &tie_total);
  const unsigned tie_room = (u64)tie_off >= keep ? 0u : (unsigned)min((u64)my_ties, keep - (u64)tie_off);
  const u64 my_mass = my_gt + (u64)tie_room * m_tau;
  u64 kept;
  const u64 m_off = block_exclusive_scan<u64>(my_mass, L.scr64, &kept);
  const u64 rnd = draw_bits(P.seed, (u64)offsets[row], (u64)(unsigned)P.stream);
  const u64 r = __umul64hi(rnd, kept);                   // uniform in [0, kept)
  if (tid == 0) L.pick = 0;                              // always defined; the owner of r overwrites it below
  __syncthreads();
  if (my_mass > 0 && r >= m_off && r < m_off + my_mass) {
    u64 run = m_off;
    unsigned ties_seen = 0;
    int pick = -1;
    for (int c = tid; c < nchunk && pick < 0; c += NT) {
      unsigned k[8];
      keys8<EDIT>(R, c, k);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        u64 m = 0;
        if (k[e] > tau) m = mass_of(R, k[e]);
        else if (k[e] == tau) { if (ties_seen < tie_room) m = m_tau; ++ties_seen; }
        if (pick < 0 && m > 0 && r < run + m) pick = 8 * c + e;
        run += m;
      }
    }
    if (pick >= 0) L.pick = pick;
  }
  __syncthreads();
  if (tid == 0) emit(L.pick);
}

// ---- history state -------------------------------------------------------------------------------------------------
__global__ void td_sampler_mark_kernel(unsigned* prompt_w, unsigned* seen_w, const int* ids, int n, int vocab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = ids[i];
  if (t < 0 || t >= vocab) return;
  atomicOr(&prompt_w[t >> 5], 1u << (t & 31));
  atomicOr(&seen_w[t >> 5], 1u << (t & 31));
}
__global__ void td_sampler_read_kernel(const uint16_t* counts, const uint8_t* prompt, int vocab, int* out_counts, uint8_t* out_mask) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= vocab) return;
  if (out_counts) out_counts[t] = (int)counts[t];
  if (out_mask) out_mask[t] = (uint8_t)((prompt[t >> 3] >> (t & 7)) & 1u);
}
__global__ void td_sampler_set_counts_kernel(uint16_t* counts, const uint8_t* prompt, uint8_t* seen, const int* in, int vocab) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;      // one byte of the bitmaps = 8 tokens
  if (c >= (vocab >> 3)) return;
  unsigned bits = 0;
  for (int e = 0; e < 8; ++e) {
    int v = in[8 * c + e];
    v = v < 0 ? 0 : (v > 65535 ? 65535 : v);
    counts[8 * c + e] = (uint16_t)v;
    bits |= (v > 0 ? 1u : 0u) << e;
  }
  seen[c] = (uint8_t)(prompt[c] | bits);
}

// ---- logit-edit state ----------------------------------------------------------------------------------------------
constexpr int BIAS_CHUNK = 256;       // table entries one launch carries in its kernel arguments (2 KiB by value: no host buffer to keep alive)
struct BiasChunk {
  int tok[BIAS_CHUNK];
  float val[BIAS_CHUNK];
};
// entries [base, base + m) of the slot's table and their bits of the bias bitmap; thread 0 of the first chunk records the table's length
__global__ void td_edits_set_bias_kernel(int* tok, float* val, int* n_out, unsigned* bias_w, const BiasChunk ch, int base, int m, int n_total) {
  const int i = threadIdx.x;
  if (i == 0 && base == 0) *n_out = n_total;
  if (i >= m) return;
  const int t = ch.tok[i];
  tok[base + i] = t;
  val[base + i] = ch.val[i];
  atomicOr(&bias_w[t >> 5], 1u << (t & 31));
}
__global__ void td_edits_ban_kernel(unsigned* ban_w, const int* ids, int n, int vocab, int on) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = ids[i];
  if (t < 0 || t >= vocab) return;
  if (on) atomicOr(&ban_w[t >> 5], 1u << (t & 31)); else atomicAnd(&ban_w[t >> 5], ~(1u << (t & 31)));
}
__global__ void td_edits_read_kernel(const uint8_t* ban, const uint8_t* bias, const int* tok, const float* val, const int* n, int vocab,
                                     uint8_t* out_ban, float* out_bias) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= vocab) return;
  if (out_ban) out_ban[t] = (uint8_t)((ban[t >> 3] >> (t & 7)) & 1u);
  if (out_bias) {
    float b = 0.f;
    if ((bias[t >> 3] >> (t & 7)) & 1u) {
      int lo = 0, hi = min(max(*n, 0), TD_MAX_LOGIT_BIAS);
      const int top = hi;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tok[mid] < t) lo = mid + 1; else hi = mid;
      }
      if (lo < top && tok[lo] == t) b = val[lo];
    }
    out_bias[t] = b;
  }
}

}  // namespace

extern "C" {

size_t td_sample_row_size(void) { return sizeof(TdSampleRow); }

int td_sampler_create(int n_slots, int vocab, td_sampler** out) {
  TD_CHECK_ARG(out, "td_sampler_create: null out");
  *out = nullptr;
  TD_CHECK_ARG(n_slots >= 1 && n_slots <= 65535, "td_sampler_create: n_slots must be in 1..65535 (got %d)", n_slots);
  TD_CHECK_ARG(vocab >= 8 && vocab % 8 == 0, "td_sampler_create: vocab must be a positive multiple of 8 (got %d)", vocab);
  td_sampler* s = new td_sampler();
  s->n_slots = n_slots;
  s->vocab = vocab;
  s->bm_stride = ((long long)(vocab / 8) + 3) / 4 * 4;
  const size_t bm = (size_t)n_slots * s->bm_stride, cn = (size_t)n_slots * vocab * sizeof(uint16_t);
  hipError_t e = hipMalloc((void**)&s->prompt, bm);
  if (e == hipSuccess) e = hipMalloc((void**)&s->seen, bm);
  if (e == hipSuccess) e = hipMalloc((void**)&s->counts, cn);
  if (e == hipSuccess) e = hipMemset(s->prompt, 0, bm);
  if (e == hipSuccess) e = hipMemset(s->seen, 0, bm);
  if (e == hipSuccess) e = hipMemset(s->counts, 0, cn);
  if (e != hipSuccess) {
    td_set_error("td_sampler_create: %s (%d slots x %d tokens)", hipGetErrorString(e), n_slots, vocab);
    td_sampler_destroy(s);
    return 3; /* TD_ERR_HIP */
  }
  *out = s;
  return 0;
}

void td_sampler_destroy(td_sampler* s) {
  if (!s) return;
  if (s->prompt) (void)hipFree(s->prompt);
  if (s->seen) (void)hipFree(s->seen);
  if (s->counts) (void)hipFree(s->counts);
  delete s;
}

#define TD_SAMPLER_SLOT(fn)                                                                                         \
  TD_CHECK_ARG(s, fn ": null sampler");                                                                             \
  TD_CHECK_ARG(slot >= 0 && slot < s->n_slots, fn ": slot %d outside [0, %d)", slot, s->n_slots)

int td_sampler_reset_slot(td_sampler* s, int slot, const int* prompt_ids_dev, int n_prompt, void* stream) {
  TD_SAMPLER_SLOT("td_sampler_reset_slot");
  TD_CHECK_ARG(n_prompt >= 0 && (n_prompt == 0 || prompt_ids_dev), "td_sampler_reset_slot: %d prompt ids with a null pointer", n_prompt);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* pr = s->prompt + (size_t)slot * s->bm_stride;
  uint8_t* se = s->seen + (size_t)slot * s->bm_stride;
  TD_CHECK_HIP(hipMemsetAsync(pr, 0, (size_t)s->bm_stride, st));
  TD_CHECK_HIP(hipMemsetAsync(se, 0, (size_t)s->bm_stride, st));
  TD_CHECK_HIP(hipMemsetAsync(s->counts + (size_t)slot * s->vocab, 0, (size_t)s->vocab * sizeof(uint16_t), st));
  if (n_prompt > 0) {
    hipLaunchKernelGGL(td_sampler_mark_kernel, dim3((n_prompt + 255) / 256), dim3(256), 0, st, (unsigned*)pr, (unsigned*)se, prompt_ids_dev, n_prompt, s->vocab);
    TD_CHECK_LAUNCH();
  }
  return 0;
}

int td_sampler_read_counts(const td_sampler* s, int slot, int32_t* out_dev, void* stream) {
  TD_SAMPLER_SLOT("td_sampler_read_counts");
  TD_CHECK_ARG(out_dev, "td_sampler_read_counts: null out");
  hipLaunchKernelGGL(td_sampler_read_kernel, dim3((s->vocab + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->counts + (size_t)slot * s->vocab,
                     s->prompt + (size_t)slot * s->bm_stride, s->vocab, out_dev, (uint8_t*)nullptr);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_sampler_read_prompt_mask(const td_sampler* s, int slot, uint8_t* out_dev, void* stream) {
  TD_SAMPLER_SLOT("td_sampler_read_prompt_mask");
  TD_CHECK_ARG(out_dev, "td_sampler_read_prompt_mask: null out");
  hipLaunchKernelGGL(td_sampler_read_kernel, dim3((s->vocab + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->counts + (size_t)slot * s->vocab,
                     s->prompt + (size_t)slot * s->bm_stride, s->vocab, (int*)nullptr, out_dev);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_sampler_set_counts(td_sampler* s, int slot, const int32_t* counts_dev, void* stream) {
  TD_SAMPLER_SLOT("td_sampler_set_counts");
  TD_CHECK_ARG(counts_dev, "td_sampler_set_counts: null counts");
  hipLaunchKernelGGL(td_sampler_set_counts_kernel, dim3((s->vocab / 8 + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->counts + (size_t)slot * s->vocab,
                     s->prompt + (size_t)slot * s->bm_stride, s->seen + (size_t)slot * s->bm_stride, counts_dev, s->vocab);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_sample_rows_bf16(const td_sampler* s, const void* logits, int64_t ld, int rows, int vocab, const TdSampleRow* params_dev,
                        const int64_t* offsets_dev, int update_state, int32_t* out_ids, void* stream) {
  TD_CHECK_ARG(logits && params_dev && offsets_dev && out_ids, "td_sample_rows_bf16: null pointer (logits %p, params %p, offsets %p, out_ids %p)",
               logits, (const void*)params_dev, (const void*)offsets_dev, (void*)out_ids);
  TD_CHECK_ARG(rows > 0 && rows <= 65535 && vocab >= 8, "td_sample_rows_bf16: need 1..65535 rows and vocab >= 8 (got %d, %d)", rows, vocab);
  TD_CHECK_ARG(vocab % 8 == 0 && ld % 8 == 0 && ld >= vocab && ((uintptr_t)logits) % 16 == 0,
               "td_sample_rows_bf16: vocab and row stride must be multiples of 8 (stride >= vocab), logits 16-byte aligned");
  TD_CHECK_ARG(!s || s->vocab == vocab, "td_sample_rows_bf16: vocab %d differs from the sampler state's %d", vocab, s ? s->vocab : 0);
  TD_CHECK_ARG(s || !update_state, "td_sample_rows_bf16: update_state needs a sampler state");
  hipLaunchKernelGGL(td_sample_rows_kernel<false>, dim3(rows), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)logits, (long long)ld, vocab, params_dev,
                     (const long long*)offsets_dev, s ? s->seen : (uint8_t*)nullptr, s ? s->counts : (uint16_t*)nullptr, s ? s->bm_stride : 0ll,
                     s ? s->n_slots : 0, update_state, out_ids, EditView{});
  TD_CHECK_LAUNCH();
  return 0;
}

// ---- logit edits ---------------------------------------------------------------------------------------------------------
int td_logit_edits_create(int n_slots, int vocab, td_logit_edits** out) {
  TD_CHECK_ARG(out, "td_logit_edits_create: null out");
  *out = nullptr;
  TD_CHECK_ARG(n_slots >= 1 && n_slots <= 65535, "td_logit_edits_create: n_slots must be in 1..65535 (got %d)", n_slots);
  TD_CHECK_ARG(vocab >= 8 && vocab % 8 == 0, "td_logit_edits_create: vocab must be a positive multiple of 8 (got %d)", vocab);
  td_logit_edits* e = new td_logit_edits();
  e->n_slots = n_slots;
  e->vocab = vocab;
  e->bm_stride = ((long long)(vocab / 8) + 3) / 4 * 4;
  const size_t bm = (size_t)n_slots * e->bm_stride, tb = (size_t)n_slots * TD_MAX_LOGIT_BIAS * 4;
  hipError_t r = hipMalloc((void**)&e->ban, bm);
  if (r == hipSuccess) r = hipMalloc((void**)&e->bias, bm);
  if (r == hipSuccess) r = hipMalloc((void**)&e->tok, tb);
  if (r == hipSuccess) r = hipMalloc((void**)&e->val, tb);
  if (r == hipSuccess) r = hipMalloc((void**)&e->n, (size_t)n_slots * sizeof(int));
  if (r == hipSuccess) r = hipMemset(e->ban, 0, bm);
  if (r == hipSuccess) r = hipMemset(e->bias, 0, bm);
  if (r == hipSuccess) r = hipMemset(e->tok, 0, tb);
  if (r == hipSuccess) r = hipMemset(e->val, 0, tb);
  if (r == hipSuccess) r = hipMemset(e->n, 0, (size_t)n_slots * sizeof(int));
  if (r != hipSuccess) {
    td_set_error("td_logit_edits_create: %s (%d slots x %d tokens)", hipGetErrorString(r), n_slots, vocab);
    td_logit_edits_destroy(e);
    return 3; /* TD_ERR_HIP */
  }
  *out = e;
  return 0;
}

void td_logit_edits_destroy(td_logit_edits* e) {
  if (!e) return;
  if (e->ban) (void)hipFree(e->ban);
  if (e->bias) (void)hipFree(e->bias);
  if (e->tok) (void)hipFree(e->tok);
  if (e->val) (void)hipFree(e->val);
  if (e->n) (void)hipFree(e->n);
  delete e;
}

#define TD_EDITS_SLOT(fn)                                                                                           \
  TD_CHECK_ARG(e, fn ": null edit state");                                                                          \
  TD_CHECK_ARG(slot >= 0 && slot < e->n_slots, fn ": slot %d outside [0, %d)", slot, e->n_slots)

int td_logit_edits_reset_slot(td_logit_edits* e, int slot, void* stream) {
  TD_EDITS_SLOT("td_logit_edits_reset_slot");
  hipStream_t st = (hipStream_t)stream;
  const size_t o = (size_t)slot * e->bm_stride;
  TD_CHECK_HIP(hipMemsetAsync(e->ban + o, 0, (size_t)e->bm_stride, st));
  TD_CHECK_HIP(hipMemsetAsync(e->bias + o, 0, (size_t)e->bm_stride, st));
  TD_CHECK_HIP(hipMemsetAsync(e->n + slot, 0, sizeof(int), st));
  return 0;
}

int td_logit_edits_set_bias(td_logit_edits* e, int slot, const int32_t* ids, const float* values, int n, void* stream) {
  TD_EDITS_SLOT("td_logit_edits_set_bias");
  TD_CHECK_ARG(n >= 0 && n <= TD_MAX_LOGIT_BIAS, "td_logit_edits_set_bias: %d entries, at most %d are held per slot", n, TD_MAX_LOGIT_BIAS);
  TD_CHECK_ARG(n == 0 || (ids && values), "td_logit_edits_set_bias: %d entries with a null pointer", n);
  int order[TD_MAX_LOGIT_BIAS];
  for (int i = 0; i < n; ++i) {
    TD_CHECK_ARG(ids[i] >= 0 && ids[i] < e->vocab, "td_logit_edits_set_bias: id %d (entry %d) outside the vocabulary [0, %d)", ids[i], i, e->vocab);
    order[i] = i;
  }
  std::sort(order, order + n, [&](int a, int b) { return ids[a] < ids[b]; });
  for (int i = 1; i < n; ++i)
    TD_CHECK_ARG(ids[order[i]] != ids[order[i - 1]], "td_logit_edits_set_bias: id %d is given twice", ids[order[i]]);
  hipStream_t st = (hipStream_t)stream;
  const size_t o = (size_t)slot * e->bm_stride;
  TD_CHECK_HIP(hipMemsetAsync(e->bias + o, 0, (size_t)e->bm_stride, st));
  TD_CHECK_HIP(hipMemsetAsync(e->n + slot, 0, sizeof(int), st));
  for (int base = 0; base < n; base += BIAS_CHUNK) {
    BiasChunk ch;
    const int m = n - base < BIAS_CHUNK ? n - base : BIAS_CHUNK;
    for (int i = 0; i < BIAS_CHUNK; ++i) {
      const float v = i < m ? values[order[base + i]] : 0.f;
      ch.tok[i] = i < m ? ids[order[base + i]] : 0;
      ch.val[i] = v != v ? 0.f : v;                                   // a NaN counts as 0
    }
    hipLaunchKernelGGL(td_edits_set_bias_kernel, dim3(1), dim3(BIAS_CHUNK), 0, st, e->tok + (size_t)slot * TD_MAX_LOGIT_BIAS,
                       e->val + (size_t)slot * TD_MAX_LOGIT_BIAS, e->n + slot, (unsigned*)(e->bias + o), ch, base, m, n);
    TD_CHECK_LAUNCH();
  }
  return 0;
}

int td_logit_edits_ban(td_logit_edits* e, int slot, const int32_t* ids_dev, int n, int on, void* stream) {
  TD_EDITS_SLOT("td_logit_edits_ban");
  TD_CHECK_ARG(n >= 0 && (n == 0 || ids_dev), "td_logit_edits_ban: %d ids with a null pointer", n);
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(td_edits_ban_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (unsigned*)(e->ban + (size_t)slot * e->bm_stride), ids_dev, n, e->vocab,
                     on ? 1 : 0);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_logit_edits_allow_only(td_logit_edits* e, int slot, const int32_t* ids_dev, int n, void* stream) {
  TD_EDITS_SLOT("td_logit_edits_allow_only");
  TD_CHECK_ARG(n >= 0 && (n == 0 || ids_dev), "td_logit_edits_allow_only: %d ids with a null pointer", n);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* bn = e->ban + (size_t)slot * e->bm_stride;
  TD_CHECK_HIP(hipMemsetAsync(bn, 0xff, (size_t)(e->vocab / 8), st));      // (the padding bytes of the stride stay 0: no token lives there)
  if (n > 0) {
    hipLaunchKernelGGL(td_edits_ban_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (unsigned*)bn, ids_dev, n, e->vocab, 0);
    TD_CHECK_LAUNCH();
  }
  return 0;
}

int td_logit_edits_read(const td_logit_edits* e, int slot, uint8_t* banned_out_dev, float* bias_out_dev, void* stream) {
  TD_EDITS_SLOT("td_logit_edits_read");
  TD_CHECK_ARG(banned_out_dev || bias_out_dev, "td_logit_edits_read: both outputs null");
  const size_t o = (size_t)slot * e->bm_stride;
  hipLaunchKernelGGL(td_edits_read_kernel, dim3((e->vocab + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->ban + o, e->bias + o,
                     e->tok + (size_t)slot * TD_MAX_LOGIT_BIAS, e->val + (size_t)slot * TD_MAX_LOGIT_BIAS, e->n + slot, e->vocab, banned_out_dev, bias_out_dev);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_sample_rows_edit_bf16(const td_sampler* s, const td_logit_edits* e, const int32_t* edit_slots_dev, const void* logits, int64_t ld, int rows,
                             int vocab, const TdSampleRow* params_dev, const int64_t* offsets_dev, int update_state, int32_t* out_ids, void* stream) {
  if (!e) return td_sample_rows_bf16(s, logits, ld, rows, vocab, params_dev, offsets_dev, update_state, out_ids, stream);
  TD_CHECK_ARG(logits && params_dev && offsets_dev && out_ids && edit_slots_dev,
               "td_sample_rows_edit_bf16: null pointer (logits %p, params %p, offsets %p, out_ids %p, edit_slots %p)", logits, (const void*)params_dev,
               (const void*)offsets_dev, (void*)out_ids, (const void*)edit_slots_dev);
  TD_CHECK_ARG(rows > 0 && rows <= 65535 && vocab >= 8, "td_sample_rows_edit_bf16: need 1..65535 rows and vocab >= 8 (got %d, %d)", rows, vocab);
  TD_CHECK_ARG(vocab % 8 == 0 && ld % 8 == 0 && ld >= vocab && ((uintptr_t)logits) % 16 == 0,
               "td_sample_rows_edit_bf16: vocab and row stride must be multiples of 8 (stride >= vocab), logits 16-byte aligned");
  TD_CHECK_ARG(!s || s->vocab == vocab, "td_sample_rows_edit_bf16: vocab %d differs from the sampler state's %d", vocab, s ? s->vocab : 0);
  TD_CHECK_ARG(e->vocab == vocab, "td_sample_rows_edit_bf16: vocab %d differs from the edit state's %d", vocab, e->vocab);
  TD_CHECK_ARG(s || !update_state, "td_sample_rows_edit_bf16: update_state needs a sampler state");
  EditView E;
  E.ban = e->ban; E.bias = e->bias; E.tok = e->tok; E.val = e->val; E.n = e->n;
  E.row_slot = edit_slots_dev; E.bm_stride = e->bm_stride; E.n_slots = e->n_slots;
  hipLaunchKernelGGL(td_sample_rows_kernel<true>, dim3(rows), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)logits, (long long)ld, vocab, params_dev,
                     (const long long*)offsets_dev, s ? s->seen : (uint8_t*)nullptr, s ? s->counts : (uint16_t*)nullptr, s ? s->bm_stride : 0ll,
                     s ? s->n_slots : 0, update_state, out_ids, E);
  TD_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
