// The e4m3 KV-cache format at the level of one 16-lane DPP row (csrc/attention_decode.hip, csrc/qwen2_engine.hip): lane j of the row holds
// elements 8j .. 8j+7 of one 128-wide head vector x as four packed bf16 pairs.
//   amax = max |x_d|;  e = the smallest integer with amax 2^-e <= 448, clamped to [-40, 40] (0 for a zero vector);
//   q_d = e4m3_rne(x_d 2^-e)  (the product is exact in fp32: one rounding);  x^_d = q_d 2^e, a bf16 value exactly.
// The weight format of csrc/quant_weight.hip applied to a head vector, through the same instructions.
#pragma once
#include "td_common.h"

// Maximum over the 16 lanes of a DPP row, every lane ending with it (row_ror 8, 4, 2, 1); all 16 lanes must be active.
__device__ __forceinline__ float kv8_row_max16(float s) {
  s = fmaxf(s, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x128, 0xf, 0xf, false)));
  s = fmaxf(s, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x124, 0xf, 0xf, false)));
  s = fmaxf(s, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x122, 0xf, 0xf, false)));
  s = fmaxf(s, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x121, 0xf, 0xf, false)));
  return s;
}

// 2^e of a vector whose largest magnitude is am (>= 0).  amax = m 2^E with m in [1, 2): amax 2^-e <= 448 = 1.75 2^8  <=>  e >= E - 8 (m <= 1.75) or
// E - 7 (m > 1.75) -- integer arithmetic on the bits, as td_quant_weight_rows_kernel does; inv = 2^-e
__device__ __forceinline__ float kv8_scale_of(float am, float& inv) {
  const unsigned ub = as_u32(am);
  int e = (int)(ub >> 23) - 127 - 8 + ((ub & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = am == 0.f ? 0 : min(max(e, -40), 40);
  inv = as_f32((unsigned)(127 - e) << 23);
  return as_f32((unsigned)(e + 127) << 23);
}

// The 8 bytes of this lane's elements under 1 / scale = inv.  The scale rule keeps every scaled value at or below 448; the clamp matters only for a vector
// whose exponent was cut off at +40, which then SATURATES at +-448.
__device__ __forceinline__ u32x2_t kv8_bytes(const u32x4_t& x, float inv) {
  unsigned b[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const unsigned u0 = x[2 * i], u1 = x[2 * i + 1];
    int word = 0;
    word = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(bf_lo(u0) * inv, -448.0f), 448.0f), fminf(fmaxf(bf_hi(u0) * inv, -448.0f), 448.0f), word, false);
    word = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(bf_lo(u1) * inv, -448.0f), 448.0f), fminf(fmaxf(bf_hi(u1) * inv, -448.0f), 448.0f), word, true);
    b[i] = (unsigned)word;
  }
  return u32x2_t{b[0], b[1]};
}

// bytes x scale -> the bf16 values q 2^e (exact: 4 significant bits, an exponent far inside bf16's range)
__device__ __forceinline__ u32x4_t kv8_to_bf16(const u32x2_t& b, float scale) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  const unsigned b0 = b[0], b1 = b[1];
  return u32x4_t{__builtin_bit_cast(unsigned, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b0, scale, false)),
                 __builtin_bit_cast(unsigned, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b0, scale, true)),
                 __builtin_bit_cast(unsigned, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b1, scale, false)),
                 __builtin_bit_cast(unsigned, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b1, scale, true))};
}

// One head vector through the format: x (this lane's 8 bf16 elements) is replaced by x^; returns the bytes and the scale (the same in all 16 lanes).
__device__ __forceinline__ u32x2_t kv8_round_row(u32x4_t& x, float& scale) {
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned u = x[i];
    am = fmaxf(am, fmaxf(fabsf(bf_lo(u)), fabsf(bf_hi(u))));
  }
  am = kv8_row_max16(am);
  float inv;
  scale = kv8_scale_of(am, inv);
  const u32x2_t b = kv8_bytes(x, inv);
  x = kv8_to_bf16(b, scale);
  return b;
}
