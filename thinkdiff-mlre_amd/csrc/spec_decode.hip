// Speculative decoding, the accept rule on the device (td_spec_accept; the rule is stated in include/thinkdiff_hip.h).
//
// A verify step feeds sequence b the rows [row0[b], row0[b] + t[b]): its last token and t[b] - 1 guessed ones.  Every row's next token has been SAMPLED
// from the target distribution (the existing sampler, one launch over all rows); a guess only decides whether the row behind it was computed on a true
// prefix.  So the sampled tokens are kept up to and including the first row whose sample differs from the guess that was fed behind it:
//   a[b] = the number of leading j < t[b] - 1 with input[row0 + j + 1] == sampled[row0 + j];   n_emit[b] = a[b] + 1;   emit[b, 0 .. a[b]] = sampled[row0 ..].
// At most 8 compares per sequence: one lane per sequence, 64 sequences per workgroup.
#include "td_common.h"
#include "td_kernels.h"
#include "../../include/thinkdiff_hip.h"

namespace {

__global__ __launch_bounds__(64) void td_spec_accept_kernel(const int* __restrict__ sampled, const int* __restrict__ input, const int* __restrict__ row0,
                                                            const int* __restrict__ rows, int B, int* __restrict__ n_emit, int* __restrict__ emit) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int t = rows[b];
  t = t < 1 ? 1 : (t > TD_MAX_VERIFY_ROWS ? TD_MAX_VERIFY_ROWS : t);
  const int r0 = row0[b];
  int a = 0;
  while (a < t - 1 && input[r0 + a + 1] == sampled[r0 + a]) ++a;
  n_emit[b] = a + 1;
  for (int j = 0; j < TD_MAX_VERIFY_ROWS; ++j) emit[b * TD_MAX_VERIFY_ROWS + j] = j <= a ? sampled[r0 + j] : -1;
}

}  // namespace

extern "C" int td_spec_accept(const int32_t* sampled, const int32_t* input, const int32_t* seq_row0, const int32_t* seq_rows, int B, int32_t* n_emit,
                              int32_t* emit, void* stream) {
  TD_CHECK_ARG(sampled && input && seq_row0 && seq_rows, "td_spec_accept: null input (sampled %p, input %p, seq_row0 %p, seq_rows %p)", (const void*)sampled,
               (const void*)input, (const void*)seq_row0, (const void*)seq_rows);
  TD_CHECK_ARG(n_emit && emit, "td_spec_accept: null output (n_emit %p, emit %p)", (void*)n_emit, (void*)emit);
  TD_CHECK_ARG(B >= 1 && B <= 256, "td_spec_accept: B=%d outside 1..256", B);
  TD_CHECK_ARG(((uintptr_t)sampled | (uintptr_t)input | (uintptr_t)seq_row0 | (uintptr_t)seq_rows | (uintptr_t)n_emit | (uintptr_t)emit) % 4 == 0,
               "td_spec_accept: every array must be 4-byte aligned");
  hipLaunchKernelGGL(td_spec_accept_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, sampled, input, seq_row0, seq_rows, B, n_emit, emit);
  TD_CHECK_LAUNCH();
  return TD_OK;
}
