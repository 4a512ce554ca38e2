// Weight-only 8-bit quantisation for the skinny-M weight streams (csrc/gemv_bf16.hip, W8 forms): the e4m3 power-of-two format of csrc/e4m3_pow2.h with
// one scale per output row of a Linear weight W[N, K].  Runs once per load (not hot); one workgroup per row, the row maximum through shuffles and LDS
// (a maximum does not depend on the order it is taken in).
#include "td_common.h"
#include "td_kernels.h"
#include "e4m3_pow2.h"
#include "mxfp4_pow2.h"

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

// The 4-bit twin: the MXFP4 format of csrc/mxfp4_pow2.h, one scale per 32 consecutive k of a row.  A thread owns a unit of 8 elements (16 bytes in, 4 bytes
// out); the 4 lanes of a block share their maximum through two shuffles.  K % 32 == 0 and the loop bound is uniform, so the 4 lanes of a block are
// always together.  Every thread reads only the elements it later overwrites, so w_hat may be w.
__global__ __launch_bounds__(QW_THREADS) void td_quant_weight_rows_mxfp4_kernel(const bf16_t* w, long long ldw, uint8_t* packed, uint8_t* scales, bf16_t* w_hat, int K) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const u32x4_t* src = (const u32x4_t*)(w + (size_t)n * ldw);
  unsigned* dq = (unsigned*)(packed + (size_t)n * (K >> 1));
  uint8_t* ds = scales + (size_t)n * (K >> 5);
  u32x4_t* dh = w_hat ? (u32x4_t*)(w_hat + (size_t)n * ldw) : nullptr;
  const int nunit = K >> 3;
  for (int c0 = 0; c0 < nunit; c0 += QW_THREADS) {
    const int c = c0 + tid;
    const bool in = c < nunit;
    const u32x4_t x = in ? src[c] : u32x4_t{0u, 0u, 0u, 0u};
    unsigned am = mx4_amax8(x, 0u);
    am = max(am, (unsigned)__shfl_xor((int)am, 1, 64));
    am = max(am, (unsigned)__shfl_xor((int)am, 2, 64));
    if (!in) continue;
    const unsigned sb = mx4_scale_byte(am);
    const unsigned b = mx4_bytes(x, mx4_inv_f32(sb));
    dq[c] = b;
    if ((c & 3) == 0) ds[c >> 2] = (uint8_t)sb;
    if (dh) dh[c] = mx4_to_bf16(b, mx4_scale_f32(sb));      // the conversion the stream kernels use: what is stored is what they will see
  }
}

__global__ __launch_bounds__(QW_THREADS) void td_dequant_rows_mxfp4_kernel(const uint8_t* packed, const uint8_t* scales, bf16_t* w_hat, long long ldw, int K) {
  const int n = blockIdx.x;
  const unsigned* sq = (const unsigned*)(packed + (size_t)n * (K >> 1));
  const uint8_t* ss = scales + (size_t)n * (K >> 5);
  u32x4_t* dh = (u32x4_t*)(w_hat + (size_t)n * ldw);
  for (int c = threadIdx.x; c < (K >> 3); c += QW_THREADS) dh[c] = mx4_to_bf16(sq[c], mx4_scale_f32(ss[c >> 2]));
}

// the shape and alignment rules both MXFP4 row entries share (`me`: the entry's name at the C ABI)
int mxfp4_rows_check(const char* me, const void* packed, const void* scales, const void* w_hat, long long ldw, int N, int K) {
  TD_CHECK_ARG(packed && scales, "%s: packed and scales are required", me);
  TD_CHECK_ARG(N > 0 && K > 0 && K % MX4_BLOCK == 0, "%s: N=%d, K=%d (K a multiple of 32, one MX block)", me, N, K);
  TD_CHECK_ARG(ldw >= K && ldw % 8 == 0 && ldw < (1ll << 31), "%s: ldw=%lld must be a multiple of 8, at least K and below 2^31", me, ldw);
  TD_CHECK_ARG((uintptr_t)w_hat % 16 == 0 && (uintptr_t)packed % 16 == 0, "%s: misaligned rows: w, w_hat and packed must be 16-byte aligned", me);
  return 0;
}

}  // namespace

int td_quant_weight_rows_mxfp4_launch(const bf16_t* w, long long ldw, uint8_t* packed, uint8_t* scales, bf16_t* w_hat, int N, int K, hipStream_t stream) {
  TD_CHECK_ARG(w, "td_quant_weight_rows_mxfp4: w is required");
  if (int rc = mxfp4_rows_check("td_quant_weight_rows_mxfp4", packed, scales, w_hat, ldw, N, K)) return rc;
  TD_CHECK_ARG((uintptr_t)w % 16 == 0, "td_quant_weight_rows_mxfp4: misaligned rows: w, w_hat and packed must be 16-byte aligned");
  hipLaunchKernelGGL(td_quant_weight_rows_mxfp4_kernel, dim3((unsigned)N), dim3(QW_THREADS), 0, stream, w, ldw, packed, scales, w_hat, K);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_dequant_rows_mxfp4_launch(const uint8_t* packed, const uint8_t* scales, bf16_t* w_hat, long long ldw, int N, int K, hipStream_t stream) {
  TD_CHECK_ARG(w_hat, "td_dequant_rows_mxfp4: w_hat is required");
  if (int rc = mxfp4_rows_check("td_dequant_rows_mxfp4", packed, scales, w_hat, ldw, N, K)) return rc;
  hipLaunchKernelGGL(td_dequant_rows_mxfp4_kernel, dim3((unsigned)N), dim3(QW_THREADS), 0, stream, packed, scales, w_hat, ldw, K);
  TD_CHECK_LAUNCH();
  return 0;
}

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
