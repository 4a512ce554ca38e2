// The e4m3 power-of-two format of the Qwen2-VL decode engine's 8-bit paths: OCP e4m3 bytes under ONE POWER-OF-TWO scale per vector x.  The vector is an
// output row of a Linear weight W[N, K] (csrc/quant_weight.hip, read by the W8 forms of csrc/gemv_bf16.hip) or one 128-wide head vector of a KV-cache
// row (csrc/attention_decode.hip, csrc/qwen2_engine.hip):
//   amax = max |x_d|;  e = the smallest integer with amax 2^-e <= 448, clamped to [-40, 40] (0 for a zero vector);
//   q_d = e4m3_rne(x_d 2^-e), saturated at +-448  (the product is exact in fp32: one rounding);  x^_d = q_d 2^e.
// A floating-point format loses nothing to a power-of-two scale, and x^ has at most 4 significant bits with an exponent far inside bf16's range, so x^ is
// a bf16 value exactly: the "8-bit model" is an ordinary bf16 model with weights W^ and a cache that holds K^ | V^.  The scale goes INTO the back-conversion
// (v_cvt_scalef32_pk_bf16_fp8 / v_cvt_scalef32_pk_f32_fp8), never onto a rounded value, and reproduces those bf16 values from the bytes.
// Everything that writes or reads the format goes through the functions below; a unit is 8 elements: four packed bf16 pairs <-> 8 bytes.
#pragma once
#include "td_common.h"

// max(am, |x_d|) over 8 bf16 elements: a vector's amax is taken 8 at a time (a maximum does not depend on the order it is taken in)
__device__ __forceinline__ float e4m3p2_amax8(const u32x4_t& x, float am) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned u = x[i];
    am = fmaxf(am, fmaxf(fabsf(bf_lo(u)), fabsf(bf_hi(u))));
  }
  return am;
}

// 2^e of a vector whose largest magnitude is am (>= 0); inv = 2^-e.  amax = m 2^E with m in [1, 2): amax 2^-e <= 448 = 1.75 2^8  <=>  e >= E - 8
// (m <= 1.75) or E - 7 (m > 1.75).  Integer arithmetic on the bits: a multiply by 1 / 448 would round, and a vector whose maximum is exactly 448 2^e must get e
__device__ __forceinline__ float e4m3p2_scale_of(float am, float& inv) {
  const unsigned ub = as_u32(am);
  int e = (int)(ub >> 23) - 127 - 8 + ((ub & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = am == 0.f ? 0 : min(max(e, -40), 40);
  inv = as_f32((unsigned)(127 - e) << 23);
  return as_f32((unsigned)(e + 127) << 23);
}

// The scale rule keeps every scaled value at or below 448, so this is the identity -- except on a vector whose exponent was clamped at +40
// (amax > 448 x 2^40: no real weight or activation), where it SATURATES to +-448 instead of leaving the out-of-range conversion to the instruction
__device__ __forceinline__ float e4m3p2_sat(float v) { return fminf(fmaxf(v, -448.0f), 448.0f); }

// 8 bf16 elements under 1 / scale = inv -> their 8 bytes
__device__ __forceinline__ u32x2_t e4m3p2_bytes(const u32x4_t& x, float inv) {
  unsigned b[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const unsigned u0 = x[2 * i], u1 = x[2 * i + 1];
    int word = 0;
    word = __builtin_amdgcn_cvt_pk_fp8_f32(e4m3p2_sat(bf_lo(u0) * inv), e4m3p2_sat(bf_hi(u0) * inv), word, false);
    word = __builtin_amdgcn_cvt_pk_fp8_f32(e4m3p2_sat(bf_lo(u1) * inv), e4m3p2_sat(bf_hi(u1) * inv), word, true);
    b[i] = (unsigned)word;
  }
  return u32x2_t{b[0], b[1]};
}

// 8 bytes x scale -> the bf16 values q 2^e, as the four packed pairs v_dot2c and the MFMA take
__device__ __forceinline__ u32x4_t e4m3p2_to_bf16(const u32x2_t& b, float scale) {
  const unsigned b0 = b[0], b1 = b[1];
  return u32x4_t{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b0, scale, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b0, scale, true)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b1, scale, false)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b1, scale, true))};
}

// 8 bytes x scale -> the same values in fp32 (what the decode attention's value accumulation takes)
__device__ __forceinline__ void e4m3p2_to_f32(const u32x2_t& b, float scale, float (&v)[8]) {
  typedef __attribute__((ext_vector_type(2))) float f32x2_t;
  const unsigned b0 = b[0], b1 = b[1];
  const f32x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(b0, scale, false), p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(b0, scale, true);
  const f32x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(b1, scale, false), p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(b1, scale, true);
  v[0] = p0[0]; v[1] = p0[1]; v[2] = p1[0]; v[3] = p1[1]; v[4] = p2[0]; v[5] = p2[1]; v[6] = p3[0]; v[7] = p3[1];
}

// One 128-wide head vector through the format at the level of a 16-lane DPP row (all 16 lanes active): lane j holds elements 8j .. 8j+7.  x is
// replaced by x^; returns this lane's bytes, and the scale (the same in all 16 lanes).
__device__ __forceinline__ u32x2_t kv8_round_row(u32x4_t& x, float& scale) {
  float inv;
  scale = e4m3p2_scale_of(row16_max(e4m3p2_amax8(x, 0.f)), inv);
  const u32x2_t b = e4m3p2_bytes(x, inv);
  x = e4m3p2_to_bf16(b, scale);
  return b;
}
