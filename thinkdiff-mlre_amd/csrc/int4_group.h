// The grouped int4 format of the Qwen2-VL decode engine's AWQ / GPTQ weight stream: asymmetric uint4 nibbles under ONE fp16 scale and ONE 4-bit zero point
// per group of G consecutive k of an output row of a Linear weight W[N, K], G in {32, 64, 128}, K % G == 0 and K % 32 == 0 (csrc/quant_weight.hip writes it
// from the two checkpoint layouts and reads it back, the I4 forms of csrc/gemv_bf16.hip stream it):
//   q, z in 0 .. 15, s a finite fp16;   w^ = bf16_rne(fp32(q - z) * fp32(s))   -- ONE rounding.
// q - z has at most 5 significant bits and s has 11, so the product is exact in fp32 (|w^| <= 15 * 65504, and the smallest non-zero magnitude 2^-24 is a
// normal fp32 and a normal bf16), and the rounding to bf16 is the only one: every reader that applies it reproduces the same bf16 value, so the "int4 model"
// is an ordinary bf16 model with weights W^, as in the e4m3 and MXFP4 modes.  The readers compute it as fma(fp32(q), s, -(fp32(z) * s)): z * s is exact
// (4 x 11 bits), and the fma rounds q s - z s = (q - z) s, which is representable, so nothing is rounded before the conversion to bf16.
// Storage: packed uint8 [N, K / 2], scales fp16 [N, K / G], zeros uint8 [N, K / G].  The order of the nibbles: packed[n, j] holds element 2j in its LOW nibble
// and 2j + 1 in its high one, so of a dword d (8 elements) the bytes of d & 0x0F0F0F0F are the even elements and those of (d >> 4) & 0x0F0F0F0F the odd ones:
// v_cvt_f32_ubyte0..3 on the two words yields the eight q as fp32, already paired (2i, 2i + 1) for the packed conversion to the bf16 pairs v_dot2c and the
// MFMA take.  Nothing outside this header assumes that order.  A unit is 8 elements (one dword <-> four bf16 pairs); a 16-byte chunk of a packed row is
// 32 elements and therefore lies inside one group.
#pragma once
#include "td_common.h"

constexpr int I4_CHUNK = 32;      // elements of a 16-byte chunk: the finest group

// log2(G) of a served group size, or 0
inline int i4_gshift_of(int G) { return G == 32 ? 5 : G == 64 ? 6 : G == 128 ? 7 : 0; }

// a group's (s, z) as the readers keep it: the fp32 scale and the fp32 offset -(z s) (exact)
struct I4Group { float s, nzs; };

__device__ __forceinline__ I4Group i4_group(unsigned scale_bits, unsigned zero) {
  const float s = (float)__builtin_bit_cast(_Float16, (unsigned short)scale_bits);
  return I4Group{s, -((float)(zero & 15u) * s)};
}

// one dword (8 elements of one group) -> the bf16 values w^ as the four packed pairs v_dot2c and the MFMA take
__device__ __forceinline__ u32x4_t i4_to_bf16(unsigned d, const I4Group& g) {
  unsigned ev = d & 0x0F0F0F0Fu, od = (d >> 4) & 0x0F0F0F0Fu;
  // (an empty statement the optimiser cannot see through: left alone it folds the masks into a shift and a mask PER ELEMENT in front of v_cvt_f32_ubyte0 --
  // three instructions a weight where v_cvt_f32_ubyte0..3 on these two words is one)
  asm volatile("" : "+v"(ev), "+v"(od));
  u32x4_t r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = (float)((ev >> (8 * i)) & 0xffu), b = (float)((od >> (8 * i)) & 0xffu);
    r[i] = pack_bf2(__builtin_fmaf(a, g.s, g.nzs), __builtin_fmaf(b, g.s, g.nzs));
  }
  return r;
}

// element j (0 .. 7) of a unit: where a writer puts its nibble in the dword
__device__ __forceinline__ unsigned i4_place(unsigned q, int j) { return (q & 15u) << (4 * j); }
