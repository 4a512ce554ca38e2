// Beam search, the step's choice on the device (td_beam_select; the rule is stated in include/thinkdiff_hip.h).
//
// A launch covers R requests of W cache rows each: row r*W + j is slot position j of request r.  Every live row brings the 2W most probable
// continuations of its beam (td_logprobs_rows_bf16 with n_top = 2W: raw logprobs in a fixed order); out of the up to W x 2W candidates the W with the
// largest cumulative logprob become the next beams, EOS candidates are set aside as finishers of their row, and the new beams are PLACED: a beam
// stays in its parent's row where it can, so that only the rows of beams that died are overwritten -- by a copy whose source no copy of the same
// step writes (td_kv_gather_rows does them all in one launch).
//
// One wave per request.  At most 200 candidates: each lane keeps ceil(200 / 64) = 4 of them in registers and counts, against all candidates in LDS,
// how many come before each of its own (a total order, so the counts are the ranks: no sort, no ties left to the hardware).  Lane 0 walks the W new
// beams twice for the placement; W lanes write the rows.  Nothing here is worth more: the step's cost is the launch.
#include "td_common.h"
#include "../../include/thinkdiff_hip.h"

namespace {

constexpr int BS_NT = 64;
constexpr int BS_MAXW = TD_MAX_BEAM_WIDTH;
constexpr int BS_MAXC = BS_MAXW * 2 * BS_MAXW;      // 200 candidates
constexpr int BS_PER = (BS_MAXC + BS_NT - 1) / BS_NT;

constexpr long long BS_NO_KEY = 0x7fffffffffffffffLL;      // the key of what is no beam candidate: behind every real one

// a before b in (cum descending, rank_in ascending, column ascending, row ascending); key = rank_in << 16 | column << 8 | row
__device__ __forceinline__ bool bs_before(float ca, long long ka, float cb, long long kb) { return ca > cb || (ca == cb && ka < kb); }

__global__ __launch_bounds__(BS_NT) void td_beam_select_kernel(const int* __restrict__ top_ids, const float* __restrict__ top_lp, int cap,
                                                               const float* __restrict__ cum_in, const int* __restrict__ rank_in, int W, int n_in, int eos,
                                                               int* __restrict__ token, float* __restrict__ cum_out, int* __restrict__ rank_out,
                                                               int* __restrict__ copy_src, int* __restrict__ parent, int* __restrict__ fin_flag,
                                                               float* __restrict__ fin_cum) {
  __shared__ float s_cum[BS_MAXC];
  __shared__ long long s_key[BS_MAXC];
  __shared__ int s_id[BS_MAXC];          // < 0: not a beam candidate (padding, EOS, a row that is not live)
  __shared__ int s_sel[BS_MAXW];         // new beam k -> its candidate, -1: missing
  __shared__ int s_beam_of_row[BS_MAXW];
  const int lane = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * W;
  const int n_cand = W * 2 * W;
  const float NEG_INF = -__builtin_huge_valf();

  for (int i = lane; i < n_cand; i += BS_NT) {
    const int j = i / (2 * W), c = i - j * 2 * W;
    int id = -1;
    float cum = NEG_INF;
    long long key = 0;
    if (j < n_in) {
      id = top_ids[(row0 + j) * cap + c];
      cum = cum_in[row0 + j] + top_lp[(row0 + j) * cap + c];
      if (!(cum == cum)) cum = NEG_INF;      // (+inf - inf: the inputs of td_logprobs_rows_bf16 cannot give it, a caller's cum_in can)
      key = ((long long)rank_in[row0 + j] << 16) | ((long long)c << 8) | j;
      if (eos >= 0 && id == eos) id = -1;
    }
    s_id[i] = id;
    s_cum[i] = id >= 0 ? cum : NEG_INF;
    s_key[i] = id >= 0 ? key : BS_NO_KEY;
  }
  if (lane < W) {
    s_sel[lane] = -1;
    // the finisher of row `lane`: its first EOS column
    int flag = 0;
    float fc = NEG_INF;
    if (lane < n_in && eos >= 0) {
      for (int c = 0; c < 2 * W && !flag; ++c) {
        if (top_ids[(row0 + lane) * cap + c] == eos) {
          flag = 1;
          fc = cum_in[row0 + lane] + top_lp[(row0 + lane) * cap + c];
          if (!(fc == fc)) fc = NEG_INF;
        }
      }
    }
    fin_flag[row0 + lane] = flag;
    fin_cum[row0 + lane] = fc;
  }
  __syncthreads();

  // the rank of each of this lane's candidates among all of them; the first W are the new beams.  One walk over the candidates in LDS (every lane
  // reads the same address: a broadcast) serves the lane's up to BS_PER candidates, which wait in registers; a candidate that is no beam
  // candidate was stored with cum -inf and the largest key, so it comes before nobody and the walk needs no third read.
  float ci[BS_PER];
  long long ki[BS_PER];
  int before[BS_PER];
#pragma unroll
  for (int u = 0; u < BS_PER; ++u) {
    const int i = lane + u * BS_NT;
    ci[u] = i < n_cand ? s_cum[i] : NEG_INF;
    ki[u] = i < n_cand ? s_key[i] : BS_NO_KEY;
    before[u] = 0;
  }
#pragma unroll 4
  for (int o = 0; o < n_cand; ++o) {
    const float co = s_cum[o];
    const long long ko = s_key[o];
#pragma unroll
    for (int u = 0; u < BS_PER; ++u) before[u] += bs_before(co, ko, ci[u], ki[u]) ? 1 : 0;
  }
#pragma unroll
  for (int u = 0; u < BS_PER; ++u) {
    const int i = lane + u * BS_NT;
    if (i < n_cand && s_id[i] >= 0 && before[u] < W) s_sel[before[u]] = i;
  }
  __syncthreads();

  // slot-stable placement: a beam whose parent's row is free keeps it, the others take the free rows in ascending order
  if (lane == 0) {
    for (int p = 0; p < W; ++p) s_beam_of_row[p] = -1;
    unsigned moved = 0;      // bit k: beam k has no row yet
    for (int k = 0; k < W; ++k) {
      const int i = s_sel[k];
      const int pj = i >= 0 ? (int)(s_key[i] & 0xff) : -1;
      if (pj >= 0 && s_beam_of_row[pj] < 0) s_beam_of_row[pj] = k;
      else moved |= 1u << k;
    }
    int next = 0;
    for (int k = 0; k < W; ++k) {
      if (moved >> k & 1u) {
        while (next < W && s_beam_of_row[next] >= 0) ++next;
        if (next < W) s_beam_of_row[next] = k;      // (W beams on W rows: there is always one)
      }
    }
  }
  __syncthreads();

  if (lane < W) {
    const int k = s_beam_of_row[lane];
    const int i = (k >= 0 && k < W) ? s_sel[k] : -1;
    const long long row = row0 + lane;
    if (i >= 0) {
      const int pj = (int)(s_key[i] & 0xff);
      token[row] = s_id[i];
      cum_out[row] = s_cum[i];
      parent[row] = (int)(row0 + pj);
      copy_src[row] = pj == lane ? -1 : (int)(row0 + pj);
    } else {      // a missing beam: fewer than W candidates
      token[row] = -1;
      cum_out[row] = NEG_INF;
      parent[row] = (int)row;
      copy_src[row] = -1;
    }
    rank_out[row] = k;
  }
}

}  // namespace

extern "C" int td_beam_select(const int32_t* top_ids, const float* top_lp, int cap, const float* cum_in, const int32_t* rank_in, int R, int W, int n_in,
                              int eos, int32_t* token, float* cum_out, int32_t* rank_out, int32_t* copy_src, int32_t* parent, int32_t* fin_flag,
                              float* fin_cum, void* stream) {
  TD_CHECK_ARG(top_ids && top_lp && cum_in && rank_in, "td_beam_select: null input (top_ids %p, top_lp %p, cum_in %p, rank_in %p)", (const void*)top_ids,
               (const void*)top_lp, (const void*)cum_in, (const void*)rank_in);
  TD_CHECK_ARG(token && cum_out && rank_out && copy_src && parent && fin_flag && fin_cum,
               "td_beam_select: null output (token %p, cum_out %p, rank_out %p, copy_src %p, parent %p, fin_flag %p, fin_cum %p)", (void*)token, (void*)cum_out,
               (void*)rank_out, (void*)copy_src, (void*)parent, (void*)fin_flag, (void*)fin_cum);
  TD_CHECK_ARG(W >= 1 && W <= TD_MAX_BEAM_WIDTH, "td_beam_select: W=%d outside 1..%d", W, TD_MAX_BEAM_WIDTH);
  TD_CHECK_ARG(cap >= 2 * W, "td_beam_select: cap=%d holds fewer than 2 W = %d columns", cap, 2 * W);
  TD_CHECK_ARG(n_in == 1 || n_in == W, "td_beam_select: n_in=%d is neither 1 (the first step) nor W=%d", n_in, W);
  TD_CHECK_ARG(R >= 1, "td_beam_select: R=%d, at least one request is needed", R);
  TD_CHECK_ARG((long long)R * W <= 65535, "td_beam_select: R*W=%lld rows exceed 65535", (long long)R * W);
  hipLaunchKernelGGL(td_beam_select_kernel, dim3(R), dim3(BS_NT), 0, (hipStream_t)stream, top_ids, top_lp, cap, cum_in, rank_in, W, n_in, eos, token, cum_out,
                     rank_out, copy_src, parent, fin_flag, fin_cum);
  TD_CHECK_LAUNCH();
  return 0;
}
