// The OCP MXFP4 format of the Qwen2-VL decode engine's 4-bit weight stream: e2m1 elements under ONE e8m0 POWER-OF-TWO scale per block of 32 consecutive k
// of an output row of a Linear weight W[N, K], K % 32 == 0 (csrc/quant_weight.hip writes it, the W4 forms of csrc/gemv_bf16.hip read it):
//   amax = max |w| over the block;  e = floor(log2(amax)) - 2 (OCP MX v1.0; 2 = emax of e2m1), clamped to [-64, 64] (0 for an all-zero block);
//   q = e2m1_rne(w 2^-e): round to nearest, ties to the even code, saturated at +-6 (the rule itself leaves scaled values in (6, 8), which clip to 6);
//   the grid is {0, 0.5, 1, 1.5, 2, 3, 4, 6} with a sign bit (-0 keeps it);  w^ = q 2^e.
// w^ has at most 2 significant bits with an exponent far inside bf16's range, so it is a bf16 value exactly: the "MXFP4 model" is an ordinary bf16 model
// with weights W^.  Storage: packed[n, j] holds element 2j in its LOW nibble and 2j + 1 in its high one; scales[n, k / 32] = e + 127 (e8m0).  The scale goes
// INTO the back-conversion (v_cvt_scalef32_pk_bf16_fp4, fp32 scale = (e + 127) << 23) and reproduces those bf16 values from the bytes.
// Everything that writes or reads the format goes through the functions below; a unit is 8 elements: four packed bf16 pairs <-> 4 bytes (one dword),
// a block is 4 units = one 16-byte chunk of a packed row.
#pragma once
#include "td_common.h"

constexpr int MX4_BLOCK = 32;      // elements under one scale

// max(am, |x_d|) over 8 bf16 elements, on the 15 magnitude bits: for finite values the order of the bits is the order of the magnitudes, and an integer
// maximum neither rounds nor flushes a subnormal
__device__ __forceinline__ unsigned mx4_amax8(const u32x4_t& x, unsigned am) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned u = x[i];
    am = max(am, max(u & 0x7fffu, (u >> 16) & 0x7fffu));
  }
  return am;
}

// the block's e8m0 byte e + 127 from the magnitude bits of its largest element: the exponent field IS floor(log2(amax)) + 127 (no log, no reciprocal)
__device__ __forceinline__ unsigned mx4_scale_byte(unsigned am) {
  const int e = (int)(am >> 7) - 127 - 2;
  return am == 0 ? 127u : (unsigned)(min(max(e, -64), 64) + 127);
}
// ... as the fp32 scale 2^e the conversion instruction takes, and its inverse 2^-e
__device__ __forceinline__ float mx4_scale_f32(unsigned sb) { return as_f32(sb << 23); }
__device__ __forceinline__ float mx4_inv_f32(unsigned sb) { return as_f32((254u - sb) << 23); }

// e2m1 code of a scaled value v = w 2^-e (exact in fp32): the grid's midpoints, each closed on the side of its even code; beyond 5 everything is 6
__device__ __forceinline__ unsigned mx4_code(float v) {
  const float a = fabsf(v);
  const unsigned c = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
  return c | ((as_u32(v) >> 28) & 8u);
}

// 8 bf16 elements under 1 / scale = inv -> their 4 bytes (element 2j in the low nibble of byte j)
__device__ __forceinline__ unsigned mx4_bytes(const u32x4_t& x, float inv) {
  unsigned b = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned u = x[i];
    b |= (mx4_code(bf_lo(u) * inv) | (mx4_code(bf_hi(u) * inv) << 4)) << (8 * i);
  }
  return b;
}

// 4 bytes x scale -> the bf16 values q 2^e, as the four packed pairs v_dot2c and the MFMA take
__device__ __forceinline__ u32x4_t mx4_to_bf16(unsigned b, float scale) {
  return u32x4_t{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(b, scale, 0)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(b, scale, 1)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(b, scale, 2)),
                 __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(b, scale, 3))};
}
