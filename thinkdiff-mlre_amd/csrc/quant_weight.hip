// Weight-only 8-bit quantisation for the skinny-M weight streams (csrc/gemv_bf16.hip, W8 forms): the e4m3 power-of-two format of csrc/e4m3_pow2.h with
// one scale per output row of a Linear weight W[N, K].  Runs once per load (not hot); one workgroup per row, the row maximum through shuffles and LDS
// (a maximum does not depend on the order it is taken in).
#include "td_common.h"
#include "td_kernels.h"
#include "e4m3_pow2.h"

namespace {

constexpr int QW_THREADS = 256;

__global__ __launch_bounds__(QW_THREADS) void td_quant_weight_rows_kernel(const bf16_t* w, long long ldw, uint8_t* q, float* scale, bf16_t* w_hat, int K) {
  __shared__ float red[QW_THREADS / 64];
  const int n = blockIdx.x, tid = threadIdx.x;
  const u32x4_t* src = (const u32x4_t*)(w + (size_t)n * ldw);
  const int nchunk = K >> 3;
  float am = 0.f;
  for (int c = tid; c < nchunk; c += QW_THREADS) am = e4m3p2_amax8(src[c], am);
  am = wave_max(am);
  if ((tid & 63) == 0) red[tid >> 6] = am;
  __syncthreads();      // (also: every read of the row for its maximum is done before anybody overwrites it -- w_hat may be w)
  am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float inv;
  const float s = e4m3p2_scale_of(am, inv);
  if (tid == 0) scale[n] = s;
  u32x2_t* dq = (u32x2_t*)(q + (size_t)n * K);
  u32x4_t* dh = w_hat ? (u32x4_t*)(w_hat + (size_t)n * ldw) : nullptr;
  for (int c = tid; c < nchunk; c += QW_THREADS) {
    const u32x2_t b = e4m3p2_bytes(src[c], inv);
    dq[c] = b;
    if (dh) dh[c] = e4m3p2_to_bf16(b, s);      // the conversion the stream kernels use: what is stored is what they will see
  }
}

}  // namespace

int td_quant_weight_rows_launch(const bf16_t* w, long long ldw, uint8_t* q, float* scale, bf16_t* w_hat, int N, int K, hipStream_t stream) {
  TD_CHECK_ARG(w && q && scale, "td_quant_weight_rows_e4m3: w, q and scale are required");
  TD_CHECK_ARG(N > 0 && K > 0 && K % 8 == 0, "td_quant_weight_rows_e4m3: N=%d, K=%d (K a multiple of 8)", N, K);
  TD_CHECK_ARG(ldw >= K && ldw % 8 == 0 && ldw < (1ll << 31), "td_quant_weight_rows_e4m3: ldw=%lld must be a multiple of 8, at least K and below 2^31", ldw);
  TD_CHECK_ARG((uintptr_t)w % 16 == 0 && (uintptr_t)w_hat % 16 == 0 && (uintptr_t)q % 8 == 0 && (uintptr_t)scale % 4 == 0,
               "td_quant_weight_rows_e4m3: misaligned rows: w and w_hat must be 16-byte aligned, q 8-byte, scale 4-byte");
  hipLaunchKernelGGL(td_quant_weight_rows_kernel, dim3((unsigned)N), dim3(QW_THREADS), 0, stream, w, ldw, q, scale, w_hat, K);
  TD_CHECK_LAUNCH();
  return 0;
}
