// Weight-only 8-bit quantisation for the skinny-M weight streams (csrc/gemv_bf16.hip, W8 forms): OCP e4m3 bytes with ONE POWER-OF-TWO scale per
// output row of a Linear weight W[N, K]:
//   amax_n = max_k |W[n, k]|;  e_n = the smallest integer with amax_n 2^-e_n <= 448, clamped to [-40, 40] (0 for an all-zero row);
//   q[n, k] = e4m3_rne(W[n, k] 2^-e_n)  (the product is exact in fp32: one rounding);  W^[n, k] = q[n, k] 2^e_n.
// A floating-point format loses nothing to a power-of-two scale, and W^ has at most 4 significant bits with an exponent far inside bf16's range, so W^ is
// a bf16 value exactly: the "8-bit model" is an ordinary bf16 model with weights W^, and v_cvt_scalef32_pk_bf16_fp8 with the row's scale reproduces
// those bf16 values from the bytes.  Runs once per load (not hot); one workgroup per row, the row maximum through shuffles and LDS (a maximum does
// not depend on the order it is taken in).
#include "td_common.h"
#include "td_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

constexpr int QW_THREADS = 256;

// The scale rule keeps every scaled weight at or below 448, so this is the identity -- except on a row whose exponent was clamped at +40
// (amax > 448 x 2^40: no real weight), where it SATURATES to +-448 instead of leaving the out-of-range conversion to the instruction
__device__ __forceinline__ float sat448(float v) { return fminf(fmaxf(v, -448.0f), 448.0f); }

__global__ __launch_bounds__(QW_THREADS) void td_quant_weight_rows_kernel(const bf16_t* w, long long ldw, uint8_t* q, float* scale, bf16_t* w_hat, int K) {
  __shared__ float red[QW_THREADS / 64];
  const int n = blockIdx.x, tid = threadIdx.x;
  const u32x4_t* src = (const u32x4_t*)(w + (size_t)n * ldw);
  const int nchunk = K >> 3;
  float am = 0.f;
  for (int c = tid; c < nchunk; c += QW_THREADS) {
    const u32x4_t v = src[c];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned u = v[i];
      am = fmaxf(am, fmaxf(fabsf(bf_lo(u)), fabsf(bf_hi(u))));
    }
  }
  am = wave_max(am);
  if ((tid & 63) == 0) red[tid >> 6] = am;
  __syncthreads();      // (also: every read of the row for its maximum is done before anybody overwrites it -- w_hat may be w)
  am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  // amax = m 2^E with m in [1, 2): amax 2^-e <= 448 = 1.75 2^8  <=>  e >= E - 8 (m <= 1.75) or E - 7 (m > 1.75).  Integer arithmetic on the bits: a
  // multiply by 1 / 448 would round, and a row whose maximum is exactly 448 2^e must get e
  const unsigned ub = as_u32(am);
  int e = (int)(ub >> 23) - 127 - 8 + ((ub & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = am == 0.f ? 0 : min(max(e, -40), 40);
  const float s = as_f32((unsigned)(e + 127) << 23), inv = as_f32((unsigned)(127 - e) << 23);
  if (tid == 0) scale[n] = s;
  u32x2_t* dq = (u32x2_t*)(q + (size_t)n * K);
  u32x4_t* dh = w_hat ? (u32x4_t*)(w_hat + (size_t)n * ldw) : nullptr;
  for (int c = tid; c < nchunk; c += QW_THREADS) {
    const u32x4_t v = src[c];
    unsigned b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned u0 = v[2 * i], u1 = v[2 * i + 1];
      int word = 0;
      word = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(bf_lo(u0) * inv), sat448(bf_hi(u0) * inv), word, false);
      word = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(bf_lo(u1) * inv), sat448(bf_hi(u1) * inv), word, true);
      b[i] = (unsigned)word;
    }
    dq[c] = u32x2_t{b[0], b[1]};
    if (dh) {      // the conversion the stream kernels use: what is stored is what they will see
      unsigned o[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        o[2 * i] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b[i], s, false));
        o[2 * i + 1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b[i], s, true));
      }
      dh[c] = u32x4_t{o[0], o[1], o[2], o[3]};
    }
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
