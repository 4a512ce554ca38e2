// Shared pieces of the gfx950 attention kernels (attention_bf16.hip: the bf16 forms; attention_fp8.hip: the e4m3 form): tile constants,
// lane-exchange helpers, the bf16 tile math (reference point and row sums on the matrix pipe; the score-bound form's 16x16x32 body), the 16-byte epilogue stores, the stream-K
// range and split-item hand-off both persistent kernels run, and the once-per-device launch helper.  Internal; included by those two files only.
#pragma once
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "td_common.h"
#include "td_kernels.h"

namespace {

constexpr int D = 128;          // head dim
constexpr int KV_TILE = 64;     // keys per iteration
constexpr int Q_WAVE = 32;      // query rows per wave
constexpr int TILE_BYTES = KV_TILE * D * 2;  // 16 KiB per K or V tile

// v_permlane32_swap a, b: lanes 32-63 of a <-> lanes 0-31 of b.  Starting from a == b == x this
// leaves a = {x.lo, x.lo}, b = {x.hi, x.hi}: every lane then sees both halves of its row.
// (Inline asm on two distinct registers: hipcc folds the builtin called with identical operands.)
__device__ __forceinline__ void half_swap(float x, float& lo, float& hi) {
  lo = x;
  hi = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo), "+v"(hi));
}
// v_max3_f32 as ONE instruction: fmaxf on MFMA outputs makes hipcc emit a canonicalising v_max per operand
__device__ __forceinline__ float max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float half_swap_max(float x) {
  float a, b;
  half_swap(x, a, b);
  return fmaxf(a, b);
}
__device__ __forceinline__ float half_swap_sum(float x) {
  float a, b;
  half_swap(x, a, b);
  return a + b;
}

// The smallest bf16-representable value >= x: a positive magnitude rounds up, a negative one is truncated.
__device__ __forceinline__ float bf16_ceil(float x) {
  const unsigned u = as_u32(x);
  return as_f32((u & 0x80000000u) ? (u & 0xffff0000u) : ((u + 0xffffu) & 0xffff0000u));
}

// compile-time loop: f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N - 1>) (inline-asm immediates need constants)
template <int N, int I = 0, typename F>
__device__ __forceinline__ void attn_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    attn_static_for<N, I + 1>(f);
  }
}
// ds_read_b64_tr_b16 as inline asm (see attn_tile_softmax_pv); the caller waits with a counted lgkmcnt before the first use
template <unsigned OFF>
__device__ __forceinline__ bf16x4_t attn_ds_read_tr16(const unsigned addr) {
  bf16x4_t v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}

// ---- the tile body shared by the two kernels -------------------------------------------------------------------------------
// Round 3: the softmax's per-score VALU work that is NOT the exponential moved onto the matrix pipe (rocprofv3 SQ counters of
// round 2: 6.0 VALU per MFMA, the SIMD's issue slots -- not the half-busy matrix pipe -- set the pace):
//  * the running reference m of a query row enters the scores INSIDE the QK^T accumulation: one extra k-step whose K-side
//    fragment is the constant column 1 and whose Q-side fragment holds -m (m is kept bf16-representable, so the product is exact;
//    softmax is invariant to the reference point, any m serves) -- the accumulator leaves the MFMA chain as s - m and the
//    per-score `fma(s, c, -m c)` disappears (32 per tile and lane), with q pre-multiplied by scale * log2(e) where its producer
//    rounds it to bf16 anyway (TdAttnParams::q_prescaled; otherwise one multiply per score remains);
//  * the row sums come from the P.V product itself: one more output row-block whose V^T rows are all ones (4 MFMAs per tile
//    into a 16-register accumulator, every register the complete sum over the 64 keys) replaces 32 adds per tile and lane and
//    the half swap at the end; the sum is over the bf16-rounded probabilities the P.V product consumes.
// Per 64-key tile and wave: 38 MFMAs (was 32) against ~32 v_exp + 16 v_cvt_pk + 16 v_max3 (+ rare rescales).
// NOREF: no reference k-step (the FIXED form: the caller's score bound keeps exp2(s) itself inside the floating-point range, so the scores
// are exponentiated as they are) -- 36 MFMAs per tile instead of 38.
template <unsigned PO, bool NOREF = false>
__device__ __forceinline__ void attn_tile_scores(f32x16_t (&st)[2], const bf16x8_t (&qf)[8], const bf16x8_t kone, const bf16x8_t qnegm,
                                                 const unsigned (&ka)[8]) {
  // K fragments are fetched KPF MFMAs ahead of their use (pinned: hipcc would issue each read right before its consumer and
  // expose the LDS latency 16 times per tile); depth re-measured in-process at S = 4289: 2 beats 4 and 6 by 2 % (1 ties)
  constexpr int KPF = 2;
  const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto kread = [&](int e) {   // e = kb * 8 + ks
    return *(const TD_LDS bf16x8_t*)(uintptr_t)(ka[e & 7] + PO + (e >> 3) * 32 * 256);
  };
  bf16x8_t kf[16];
#pragma unroll
  for (int e = 0; e < KPF; ++e) kf[e] = kread(e);
  __builtin_amdgcn_sched_group_barrier(0x100, KPF, 0);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (!NOREF && (e & 7) == 0) {      // the reference point first: st = 1 . (-m)
      st[e >> 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kone, qnegm, zero16, 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    }
    if (e + KPF < 16) kf[e + KPF] = kread(e + KPF);
    st[e >> 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[e], qf[e & 7], (NOREF && (e & 7) == 0) ? zero16 : st[e >> 3], 0, 0, 0);
    if (e + KPF < 16) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  }
}

// st holds s - m_run (raw score units; log2 units when PRE).  `first`: the first tile of this (part of an) item -- o, lacc are
// zero and m_run is 0: the reference point is set to the tile's row maximum whatever it is.
// RS: row sums on the matrix pipe (lacc); otherwise they are added on the VALU into lacc[0] as HALF sums (the caller adds the
// two lane halves at the end) -- the A/B of which pipe has room on a given shape.
// FIXED: the caller knows a bound of every score (TdAttnParams::score_bound <= 48 octaves): the scores are exponentiated as they are -- no row
// maximum, no branch, no rescale, no reference at all (m_run = 0).  A bf16 probability keeps its 8 mantissa bits at any magnitude and the sums
// are fp32: exp2(s) <= 2^48, a row sum <= 2^61, and exp2(s) >= 2^-48 (|s| <= bound) -- all far inside the floating-point range.
template <unsigned PO, bool PRE, bool RS = true, bool FIXED = false>
__device__ __forceinline__ void attn_tile_softmax_pv(f32x16_t (&st)[2], f32x16_t (&o)[4], f32x16_t& lacc, float& m_run, bf16x8_t& qnegm,
                                                     const bool first, const float c, const unsigned (&va)[2][4], const int h5) {
  const float cc = PRE ? 1.0f : c;
  if constexpr (!FIXED) {
  // The FIRST read of the fresh QK^T accumulators is one the compiler can see (fmaxf): its hazard recogniser then places the wait states a
  // VALU read of a 16-pass MFMA result needs.  Inline-asm v_max3 alone is invisible to it and may read registers the matrix pipe has
  // not written yet (csrc/attention_fp8.hip met exactly that: a row maximum that missed elements, about one row in 600).
  float mx = fmaxf(st[0][15], st[1][15]);
#pragma unroll
  for (int r = 0; r < 15; ++r) mx = max3(mx, st[0][r], st[1][r]);
  mx = half_swap_max(mx);
  constexpr float RESCALE_LOG2 = 8.0f;        // deferred rescale: probabilities may reach 2^8 before the reference moves
  if (first || __any(mx * cc > RESCALE_LOG2)) {
    float target = first ? mx : fmaxf(mx, 0.f);             // new reference relative to the old one
    if (!(target > -INFINITY)) target = 0.f;                  // a fully masked row keeps its reference
    const float m_new = bf16_ceil(m_run + target);
    const float d = m_new - m_run;                            // exact: both are short bf16 values
    if (!first) {
      const float alpha = __builtin_amdgcn_exp2f(-d * cc);
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      if constexpr (RS) {
#pragma unroll
        for (int r = 0; r < 16; ++r) lacc[r] *= alpha;
      } else lacc[0] *= alpha;
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[kb][r] -= d;
    m_run = m_new;
    qnegm[0] = h5 == 0 ? (short)f2bf(-m_new) : (short)0;
  }
  }      // (!FIXED)
  bf16x8_t pf[2][2];
  float psum = 0.f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4_t pk;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = st[kb][8 * s + 2 * j], x1 = st[kb][8 * s + 2 * j + 1];
        const float p0 = __builtin_amdgcn_exp2f(PRE ? x0 : x0 * c);
        const float p1 = __builtin_amdgcn_exp2f(PRE ? x1 : x1 * c);
        if constexpr (!RS) psum += p0 + p1;
        pk[j] = pack_bf2(p0, p1);
      }
      pf[kb][s] = __builtin_bit_cast(bf16x8_t, pk);
    }
  }
  if constexpr (!RS) lacc[0] += psum;

  // ---- O^T += V^T . P^T, and the row sums as one more row-block of ones ---------------------------------------------------
  // The transposed V^T reads are INLINE ASM, with their own counted waits: behind an LDS-DMA in flight hipcc puts `s_waitcnt vmcnt(0)`
  // in front of the first __builtin_amdgcn_ds_read_tr16_b64 (its memory operand may alias the DMA's destination as far as the
  // compiler can tell; plain loads through an integer-cast address carry no such operand and are left alone), i.e. every wave waited
  // for the NEXT tile's K | V in the middle of the running tile -- and the two-slot kernels had come to RELY on that wait (see their tile top).  LDS operations of a wave complete in order,
  // so `lgkmcnt(n)` with n = the reads issued behind the wanted pair is exact, and a compiler-inserted wait that does not know of
  // these reads can only wait longer than it means to.  The wait carries the fragment as an in/out operand so that its MFMA cannot
  // be scheduled above it; sched_barrier pins the read / wait / MFMA order (VALU and SALU work may still move across).
  constexpr int VPF = 2;   // V^T fragments in flight ahead of their MFMA (2 transposed reads each)
  const bf16x8_t ones8 = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  bf16x4_t v0[16], v1[16];
  attn_static_for<VPF>([&](auto ec) {
    constexpr int e = decltype(ec)::value;
    v0[e] = attn_ds_read_tr16<PO + (e >> 2) * 16 * 256>(va[0][e & 3]);
    v1[e] = attn_ds_read_tr16<PO + (e >> 2) * 16 * 256>(va[1][e & 3]);
  });
  attn_static_for<16>([&](auto ec) {
    constexpr int e = decltype(ec)::value;
    if constexpr (e + VPF < 16) {
      v0[e + VPF] = attn_ds_read_tr16<PO + ((e + VPF) >> 2) * 16 * 256>(va[0][(e + VPF) & 3]);
      v1[e + VPF] = attn_ds_read_tr16<PO + ((e + VPF) >> 2) * 16 * 256>(va[1][(e + VPF) & 3]);
    }
    constexpr int behind = 2 * (15 - e < VPF ? 15 - e : VPF);      // transposed reads issued behind pair e
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(v0[e]), "+v"(v1[e]) : "n"(behind));
    bf16x8_t vf;
    vf[0] = v0[e][0]; vf[1] = v0[e][1]; vf[2] = v0[e][2]; vf[3] = v0[e][3];
    vf[4] = v1[e][0]; vf[5] = v1[e][1]; vf[6] = v1[e][2]; vf[7] = v1[e][3];
    o[e & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[e >> 3][(e >> 2) & 1], o[e & 3], 0, 0, 0);
    if constexpr (RS && (e & 3) == 3) lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones8, pf[e >> 3][(e >> 2) & 1], lacc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0x006);
  });
}

// Normalise and store one wave's 32 x 128 output tile.  A lane holds O[q][db*32 + 8 g + 4 h5 + (0..3)] for g = 0..3: with the two
// lane halves of a row exchanged pairwise (v_permlane32_swap: upper half of group g <-> lower half of group g+1) every lane owns 8
// contiguous columns = one 16-byte store, 8 per lane instead of 16 of 8 bytes: the store tail of an attention workgroup is bound
// by the number of store instructions, not by bytes (guide, T21).
// `live`: the lane's row exists (rows past Sq take part in the lane exchange -- the swap needs both halves -- and skip the store).
__device__ __forceinline__ void attn_store_rows(const f32x16_t (&o)[4], const float inv, bf16_t* row_ptr, const int h5, const bool wide, const bool live) {
  if (wide) {
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g = 0; g < 4; g += 2) {
        unsigned a0 = pack_bf2(o[db][4 * g] * inv, o[db][4 * g + 1] * inv), a1 = pack_bf2(o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv);
        unsigned b0 = pack_bf2(o[db][4 * g + 4] * inv, o[db][4 * g + 5] * inv), b1 = pack_bf2(o[db][4 * g + 6] * inv, o[db][4 * g + 7] * inv);
        const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        const u32x4_t w = {r0[0], r1[0], r0[1], r1[1]};
        if (live) *(u32x4_t*)(row_ptr + db * 32 + 8 * (g + h5)) = w;
      }
  } else {
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u32x2_t w;
        w[0] = pack_bf2(o[db][4 * g] * inv, o[db][4 * g + 1] * inv);
        w[1] = pack_bf2(o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv);
        if (live) *(u32x2_t*)(row_ptr + 4 * h5 + db * 32 + 8 * g) = w;
      }
  }
}

// The same tile as symmetric int8 under a per-row scale fixed in advance (the FLUX engine's history-scaled int8 mode: the attention output
// is the A operand of the next int8 GEMM): q = clamp(rint(bf16(o * inv) * qinv), +-127), 8 contiguous bytes per lane after the same pairwise
// lane exchange, and the row-head maximum of |bf16(o * inv)| joins amax (atomic max on the float bits; lanes of the lower half only).
__device__ __forceinline__ void attn_store_rows_q8(const f32x16_t (&o)[4], const float inv, uint8_t* row_ptr, const int h5, const float qinv, unsigned* amax,
                                                   const bool live) {
  float am = 0.f;
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      unsigned w[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        unsigned acc = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float v = rbf(o[db][4 * (g + h) + b] * inv);          // the attention output is a bf16 tensor in the reference graph
          am = fmaxf(am, fabsf(v));
          acc |= ((unsigned)__float2int_rn(fminf(fmaxf(v * qinv, -127.f), 127.f)) & 0xffu) << (8 * b);
        }
        w[h] = acc;
      }
      const auto r = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);
      if (live) *(u32x2_t*)(row_ptr + db * 32 + 8 * (g + h5)) = u32x2_t{r[0], r[1]};
    }
  am = half_swap_max(am);
  if (live && h5 == 0) __hip_atomic_fetch_max(amax, as_u32(am), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the FIXED form's tile body on v_mfma_f32_16x16x32_bf16 (M16) -----------------------------------------------------------------
// The score-bound form has no row maximum and no rescale: its softmax is elementwise (exp2, pack) and its row sums come from the matrix
// pipe, so nothing in it needs a query row on one lane pair.  It runs both products on the 16x16x32 shape (csrc/ip_attention.hip's
// layout), which holds a higher rate under the chip's power limit than 32x32x16 and halves the share of the row-sum MFMAs (4 of
// 68 half-length MFMAs per 64-key tile and wave instead of 4 of 36).  A wave still owns 32 query rows, as two blocks qb of 16; lane =
// 16 g + i16.  Per 64-key tile:
//  * S^T[16 keys][16 q] = K . Q^T, key block kb (4), q block qb (2), 4 k-steps: 32 MFMAs into 8 accumulators, k-step outer so that
//    consecutive MFMAs write different accumulators.  Lane group g contracts head columns 32 g + 8 ks + (0..7) at k-step ks (any map the
//    two operands share serves), so q is 64 contiguous bytes per lane and q block, and a K fragment is one ds_read_b128 of 16-byte chunk
//    4 g + ks of key row 16 kb + i16 -- 16 reads per tile, each used for both q blocks.  Bank pattern in the shared 256-byte XOR image
//    (physical chunk = chunk ^ swz(row), swz = (row&3)<<2 | (row>>2)&3): ds_read_b128 is served in the 16-lane groups {0-3, 12-15, 20-27},
//    {4-11, 16-19, 28-31} and their upper-half twins, i.e. rows with (row>>2) in {0, 3} of one g next to rows with (row>>2) in {1, 2} of
//    g ^ 1.  Their chunks differ in the upper two bits only (4 g + ks), the low two bits are ks ^ (row>>2) = all four values, and under each
//    of them the upper two bits g ^ (row&3) take four values: 16 distinct 16-byte slots, conflict-free.  (With chunk 4 ks + g, the plain
//    k order, the same groups are 2-way.)
//  * accumulator register i of lane group g of block (kb, qb) is key 16 kb + 4 g + i against query 16 qb + i16.  exp2 and the bf16 pack are
//    elementwise; the packed registers of key blocks 2u and 2u + 1 side by side ARE the B operand of P.V for key pair u: k-slot 8 g + j is
//    key 32 u + 4 g + j (j < 4) or 32 u + 16 + 4 g + j - 4.
//  * O^T[16 d][16 q] += V^T . P^T, d block dt (8), q block qb, key pair u: 32 MFMAs into 64 registers, and ones . P^T per (qb, u) into
//    4 registers per q block, every register the row's complete sum.  A V^T fragment is two ds_read_b64_tr_b16 16 key rows apart (lane
//    4 q' + pb of a 16-lane group supplies key row 4 g + q', four head columns), each fragment used for both q blocks.  Operand row 4 pb + r
//    of d block dt is head column 32 pb + 4 (dt ^ (pb & 1)) + r: a lane ends with the 32 contiguous columns 32 g .. 32 g + 31 of its two
//    query rows (16-byte stores, 8 per lane, no lane exchange), the two 4-column halves of each 16 bytes swapped in the odd lane groups.
//    That swap is what makes the transposed reads conflict-free: all lanes of a 32-lane half read 8 bytes, and if all took the same half of
//    their 16-byte chunk only 16 of the 32 8-byte bank slots could be hit.  The shared image cannot serve these reads (slot
//    (pb ^ q') << 2 | ..: four key rows on one slot, 4-way), and K and V are staged by separate LDS-DMA instructions, so V takes its own
//    source-side XOR: physical chunk = chunk ^ (row & 15).  A lane then reads slot ((pb ^ g) << 2) | ((dt >> 1) ^ q'), half (dt ^ pb) & 1:
//    over a half's (g & 1, q', pb) that is a bijection onto the 32 8-byte slots of the 256-byte bank row.
constexpr int M16_FORCE_32 = 0x400;      // TdAttnParams::variant bit: the FIXED form runs the 32x32x16 body (in-process A/B)

// chunk of the source row that LDS-DMA lane `lane` of 4-row group `grp` fetches into V's image (K's: see the kernels' voffK)
__device__ __forceinline__ int attn16_v_src_chunk(const int grp, const int lane) { return (lane & 15) ^ (((grp & 3) << 2) | (lane >> 4)); }

// resident per-lane LDS byte addresses of slot 0: ka[ks] (key block and tile slot are immediates), va[dt] (key pair, fragment half, tile slot)
__device__ __forceinline__ void attn16_lds_addrs(const unsigned lds0, const int lane, unsigned (&ka)[4], unsigned (&va)[8]) {
  const unsigned i16 = lane & 15, g = lane >> 4;
  const unsigned ksw = ((i16 & 3) << 2) | (i16 >> 2);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) ka[ks] = lds0 + i16 * 256 + (((4 * g + ks) ^ ksw) << 4);
  const unsigned vq = i16 >> 2, pb = i16 & 3;
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
    va[dt] = lds0 + 2 * TILE_BYTES + (4 * g + vq) * 256 + ((((pb ^ g) << 2) | ((dt >> 1) ^ vq)) << 4) + 8 * ((dt ^ pb) & 1);
}

// q fragments of the wave's two 16-row blocks from row q0: [qb][ks] = head columns 32 g + 8 ks .. + 7 of row q0 + 16 qb + i16 (rows past the
// descriptor's range read as zeros)
__device__ __forceinline__ void attn16_load_q(bf16x8_t (&qf)[2][4], const __amdgpu_buffer_rsrc_t rsQ, const int q0, const int head, const int ldq, const int lane) {
  const unsigned qoff = (unsigned)(q0 + (lane & 15)) * (unsigned)ldq * 2u + (unsigned)(head * D + 32 * (lane >> 4)) * 2u;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      qf[qb][ks] = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rsQ, qoff + (unsigned)qb * 16u * (unsigned)ldq * 2u + ks * 16, 0, 0));
}

template <unsigned PO>
__device__ __forceinline__ void attn16_tile_scores(f32x4_t (&st)[4][2], const bf16x8_t (&qf)[2][4], const unsigned (&ka)[4]) {
  constexpr int KPF = 2;      // K fragments in flight ahead of their MFMA pair, pinned as in attn_tile_scores
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  auto kread = [&](int e) {   // e = ks * 4 + kb
    return *(const TD_LDS bf16x8_t*)(uintptr_t)(ka[e >> 2] + PO + (e & 3) * 16 * 256);
  };
  bf16x8_t kf[16];
#pragma unroll
  for (int e = 0; e < KPF; ++e) kf[e] = kread(e);
  __builtin_amdgcn_sched_group_barrier(0x100, KPF, 0);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (e + KPF < 16) kf[e + KPF] = kread(e + KPF);
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
      st[e & 3][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[e], qf[qb][e >> 2], e < 4 ? zero4 : st[e & 3][qb], 0, 0, 0);
    if (e + KPF < 16) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
  }
}

// st: the tile's scores in log2 units (q pre-scaled), exponentiated as they are.  The first VALU read of the fresh accumulators is the exp2
// builtin, which the compiler's hazard recogniser sees (see attn_tile_softmax_pv on what an inline-asm first read can miss).
template <unsigned PO>
__device__ __forceinline__ void attn16_tile_softmax_pv(const f32x4_t (&st)[4][2], f32x4_t (&o)[8][2], f32x4_t (&ls)[2], const unsigned (&va)[8]) {
  bf16x8_t pf[2][2];      // [key pair u][qb]
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      u32x4_t pk;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4_t s = st[2 * u + h][qb];
        pk[2 * h] = pack_bf2(__builtin_amdgcn_exp2f(s[0]), __builtin_amdgcn_exp2f(s[1]));
        pk[2 * h + 1] = pack_bf2(__builtin_amdgcn_exp2f(s[2]), __builtin_amdgcn_exp2f(s[3]));
      }
      pf[u][qb] = __builtin_bit_cast(bf16x8_t, pk);
    }
  // transposed reads as inline asm with counted waits, pinned read / wait / MFMA order: as attn_tile_softmax_pv, fragment e = 8 u + dt
  constexpr int VPF = 2;
  const bf16x8_t ones8 = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  bf16x4_t v0[16], v1[16];
  attn_static_for<VPF>([&](auto ec) {
    constexpr int e = decltype(ec)::value;
    v0[e] = attn_ds_read_tr16<PO + (e >> 3) * 32 * 256>(va[e & 7]);
    v1[e] = attn_ds_read_tr16<PO + (e >> 3) * 32 * 256 + 16 * 256>(va[e & 7]);
  });
  attn_static_for<16>([&](auto ec) {
    constexpr int e = decltype(ec)::value;
    if constexpr (e + VPF < 16) {
      v0[e + VPF] = attn_ds_read_tr16<PO + ((e + VPF) >> 3) * 32 * 256>(va[(e + VPF) & 7]);
      v1[e + VPF] = attn_ds_read_tr16<PO + ((e + VPF) >> 3) * 32 * 256 + 16 * 256>(va[(e + VPF) & 7]);
    }
    constexpr int behind = 2 * (15 - e < VPF ? 15 - e : VPF);      // transposed reads issued behind pair e
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(v0[e]), "+v"(v1[e]) : "n"(behind));
    const bf16x8_t vf = __builtin_shufflevector(v0[e], v1[e], 0, 1, 2, 3, 4, 5, 6, 7);
    o[e & 7][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[e >> 3][0], o[e & 7][0], 0, 0, 0);
    o[e & 7][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[e >> 3][1], o[e & 7][1], 0, 0, 0);
    if constexpr ((e & 3) == 3) ls[(e >> 2) & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones8, pf[e >> 3][(e >> 2) & 1], ls[(e >> 2) & 1], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0x006);
  });
}

// KV tiles [kb, ke) of one item, double buffered: stage(slot, t) starts tile t's LDS-DMA into `slot`; the caller has staged tile kb into slot 0
template <typename STAGE>
__device__ __forceinline__ void attn16_run_tiles(f32x4_t (&o)[8][2], f32x4_t (&ls)[2], const bf16x8_t (&qf)[2][4], const unsigned (&ka)[4], const unsigned (&va)[8],
                                                 const int kb, const int ke, const int Skv, const int lane, STAGE&& stage) {
  auto tile = [&](const int t, auto slot_tag) {
    constexpr unsigned SLOT = decltype(slot_tag)::value;
    constexpr unsigned PO = SLOT * TILE_BYTES;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my pieces of tile t landed (explicit: see the plain-grid kernel) ...
    __syncthreads();                                        // ... and everyone's; the other slot is no longer read
    if (t + 1 < ke) stage(SLOT ^ 1, t + 1);
    f32x4_t st[4][2];
    attn16_tile_scores<PO>(st, qf, ka);
    const int key0 = t * KV_TILE + 4 * (lane >> 4);
    if (t * KV_TILE + KV_TILE > Skv) {      // last tile: keys >= Skv are masked
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (key0 + 16 * kk + i >= Skv) st[kk][qb][i] = -INFINITY;
    }
    attn16_tile_softmax_pv<PO>(st, o, ls, va);
  };
  int t = kb;
  for (; t + 1 < ke; t += 2) {
    tile(t, std::integral_constant<unsigned, 0>{});
    tile(t + 1, std::integral_constant<unsigned, 1>{});
  }
  if (t < ke) tile(t, std::integral_constant<unsigned, 0>{});
}

// Normalise and store the wave's rows from q0: lane group g holds head columns 32 g + 4 (dt ^ (g & 1)) + (0..3) of rows q0 + 16 qb + i16 in o[dt][qb].
// `wide`: 16-byte stores (rows are 16-byte multiples), else 8-byte ones.  Oh: the item's output at its head's first column.
__device__ __forceinline__ void attn16_store_rows(const f32x4_t (&o)[8][2], const float (&l)[2], bf16_t* Oh, const int ldo, const int q0, const int Sq, const int lane,
                                                  const bool wide) {
  const int g = lane >> 4;
  const bool odd = g & 1;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int q = q0 + 16 * qb + (lane & 15);
    const float inv = 1.0f / l[qb];
    bf16_t* const row_ptr = Oh + (size_t)min(q, Sq - 1) * ldo + 32 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4_t a = o[2 * c][qb], b = o[2 * c + 1][qb];
      const unsigned a0 = pack_bf2(a[0] * inv, a[1] * inv), a1 = pack_bf2(a[2] * inv, a[3] * inv);
      const unsigned b0 = pack_bf2(b[0] * inv, b[1] * inv), b1 = pack_bf2(b[2] * inv, b[3] * inv);
      const u32x4_t w = {odd ? b0 : a0, odd ? b1 : a1, odd ? a0 : b0, odd ? a1 : b1};
      if (q < Sq) {
        if (wide) *(u32x4_t*)(row_ptr + 8 * c) = w;
        else { *(u32x2_t*)(row_ptr + 8 * c) = u32x2_t{w[0], w[1]}; *(u32x2_t*)(row_ptr + 8 * c + 4) = u32x2_t{w[2], w[3]}; }
      }
    }
  }
}

// ---- stream-K: the range of a persistent workgroup and the hand-off of an item split over two of them ---------------------------
// (the structure and the reasons are told in front of td_attn_fwd_d128_streamk_kernel, attention_bf16.hip)
constexpr int SK_SLOT_FLOATS = 8 * 64 * 68;          // per boundary and side: 8 waves x 64 lanes x (64 O + m + l + 2 pad) floats
constexpr int SK_HEADER_BYTES = 4096;                 // cnt[j] at word 16 + j
constexpr int SK_MAX_RANGES = SK_HEADER_BYTES / 4 - 16;
// workspace = [header | T slots: ranges x SK_SLOT_FLOATS | H slots: ranges x SK_SLOT_FLOATS]

// Logical range r of this workgroup and its (item, KV tile) iterations [it, it_end) out of `total`: with XCD_REMAP, workgroups that
// share an XCD (equal blockIdx % 8 under round-robin placement; speed only) take neighbouring ranges = neighbouring query tiles of
// the same heads = the same K/V in that L2
template <bool XCD_REMAP>
__device__ __forceinline__ int attn_sk_range(const long long total, long long& it, long long& it_end) {
  const int G = gridDim.x;
  int r = blockIdx.x;
  if constexpr (XCD_REMAP) {
    const int q8 = G >> 3, r8 = G & 7, xcd = r & 7;
    r = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (r >> 3);
  }
  it = total * r / G;
  it_end = total * (r + 1) / G;
  return r;
}

// What happens to the un-normalised state (o, m_run, l_run) of a PART of an item run by range r of G: leave it for the other owner
// (returns false: this workgroup is done with the item) or combine it with the other owner's (returns true: o and l_run are the
// whole item's, the caller normalises and stores).  `tail`: this is the item's tail part (KV tiles kb > 0 .. nt), met first by its
// range; otherwise the head part (0 .. ke < nt), met last.  cc: scale of the stored reference points (1 when they are log2 units).
// SUMS2 (the M16 body, FIXED form: no reference point): m_run is the row sum of the lane's SECOND query row, o_io any fixed order of the 64
// accumulator registers -- both owners run the same body -- and the merge is a plain add of everything.
template <bool SUMS2 = false>
__device__ __forceinline__ bool attn_sk_handoff(f32x16_t (&o_io)[4], float& m_run, float& l_run, const float cc, const int r, const int G,
                                                const bool tail, char* ws, TD_LDS unsigned* const ticket_lds, const int tid, const int wid) {
  const int lane = tid & 63;
  // (a copy: indexing the caller's array through the reference cost the e4m3 kernels 400-600 spilled VGPRs, profiles/attention_one_item_body.md)
  f32x16_t o[4] = {o_io[0], o_io[1], o_io[2], o_io[3]};
  unsigned* const cnt = (unsigned*)ws + 16;
  const int j = tail ? r : r + 1;                    // boundary between ranges j-1 (head part) and j (tail part)
  const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void*)(ws + SK_HEADER_BYTES), 0, (unsigned)(2 * G) * SK_SLOT_FLOATS * 4u, 0x00020000);
  const unsigned lane_off = ((unsigned)wid * 17u * 64u + (unsigned)lane) * 16u;      // [wave][chunk 0..16][lane] x 16 bytes
  const unsigned mine = (unsigned)(tail ? j : G + j) * (SK_SLOT_FLOATS * 4u) + lane_off;      // T[j] / H[j]
  const unsigned theirs = (unsigned)(tail ? G + j : j) * (SK_SLOT_FLOATS * 4u) + lane_off;
  // one lane asks, everyone hears the answer through LDS (block-uniform control flow below)
  auto ask = [&](bool draw) -> unsigned {
    __syncthreads();
    if (tid == 0)
      *ticket_lds = draw ? __hip_atomic_fetch_add(cnt + j, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                         : __hip_atomic_load(cnt + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return *ticket_lds;
  };
  bool other_ready = !tail && ask(false) == 1u;      // head part: the tail part's owner has normally long been through
  if (!other_ready) {
    // leave the state for the other owner: write-through stores, drained by every wave, then the ticket
#pragma unroll
    for (int q4 = 0; q4 < 16; ++q4) {
      const u32x4_t v = {as_u32(o[q4 >> 2][4 * (q4 & 3)]), as_u32(o[q4 >> 2][4 * (q4 & 3) + 1]),
                         as_u32(o[q4 >> 2][4 * (q4 & 3) + 2]), as_u32(o[q4 >> 2][4 * (q4 & 3) + 3])};
      __builtin_amdgcn_raw_buffer_store_b128(v, rsS, mine + q4 * 1024u, 0, 16);       // aux 16 = sc1
    }
    const u32x4_t ml = {as_u32(m_run), as_u32(l_run), 0u, 0u};
    __builtin_amdgcn_raw_buffer_store_b128(ml, rsS, mine + 16 * 1024u, 0, 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    other_ready = ask(true) == 1u;                   // the barrier inside orders every wave's drain before the add
    if (!other_ready) return false;                  // first to arrive: the other owner finishes the item
  }
  // second to arrive: the other state is complete and published before the atomic that told us
  if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const u32x4_t ml = __builtin_amdgcn_raw_buffer_load_b128(rsS, theirs + 16 * 1024u, 0, 0);
  const float m2 = as_f32(ml[0]), l2 = as_f32(ml[1]);
  const float mm = fmaxf(m_run, m2);
  const float a1 = __builtin_amdgcn_exp2f((m_run - mm) * cc), a2 = __builtin_amdgcn_exp2f((m2 - mm) * cc);
  // One operation order whoever merges -- fma(head, a_head, tail * a_tail) -- so the result does not depend on which owner
  // arrived second (it does under load; the sum is otherwise the same to one fp32 rounding).
  auto comb = [&](float own, float other) {
    if constexpr (SUMS2) return own + other;
    return tail ? __builtin_fmaf(other, a2, own * a1) : __builtin_fmaf(own, a1, other * a2);
  };
  l_run = comb(l_run, l2);
  if constexpr (SUMS2) m_run = comb(m_run, m2);
#pragma unroll
  for (int q4 = 0; q4 < 16; ++q4) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsS, theirs + q4 * 1024u, 0, 0);
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4)
      o[q4 >> 2][4 * (q4 & 3) + k4] = comb(o[q4 >> 2][4 * (q4 & 3) + k4], as_f32(v[k4]));
  }
  if (tid == 0) __hip_atomic_store(cnt + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // both tickets drawn: ready for the next launch
#pragma unroll
  for (int db = 0; db < 4; ++db) o_io[db] = o[db];
  return true;
}

// Launch KERNEL with `lds` bytes of dynamic LDS, raising its LDS limit first, once per device: every kernel instantiation has its own
// flag word (bit d = done on device d) in its instantiation of this template.  The caller checks the launch (TD_CHECK_LAUNCH).
template <auto KERNEL, typename... Args>
int attn_launch(const dim3 grid, const int threads, const int lds, hipStream_t stream, const int dev, Args... args) {
  static std::atomic<unsigned long long> done{0};
  if (!((done.load(std::memory_order_acquire) >> (dev & 63)) & 1ull)) {
    TD_CHECK_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    done.fetch_or(1ull << (dev & 63), std::memory_order_release);
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(threads), lds, stream, args...);
  return 0;
}

}  // namespace
