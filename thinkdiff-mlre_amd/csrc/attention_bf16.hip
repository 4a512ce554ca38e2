// Flash-style fused attention forward for gfx950, head_dim = 128, bf16 in/out, fp32 softmax state.
//
// Serves K11: FLUX joint attention over [text || image] tokens (non-causal, no
// mask, 24 heads, S ~ 4.3k) and K19: Qwen2-VL prefill attention (causal, GQA 28q/4kv).
// Replaces F.scaled_dot_product_attention inside [ext] diffusers FluxAttnProcessor2_0 /
// FluxSingleAttnProcessor2_0 and the vLLM fork's Qwen2-VL attention.
//
// Structure (cdna_hip_programming guide, Appendix B "Fused attention prefill"):
//  * workgroup = 8 waves, each wave owns 32 query rows (256 rows / workgroup); KV tile = 64 keys.
//  * swapped QK^T: S^T[key][q] = K . Q^T on v_mfma_f32_32x32x16_bf16, so one query row lives on
//    one lane (and its lane+32 partner): the online softmax is in-register, the row max / row sum
//    need one half-swap (v_permlane32_swap) and no LDS.
//  * the S^T accumulator, converted to bf16 in place, IS the B operand of the P.V product
//    (O^T[d][q] += V^T[d][key] . P^T[key][q]); V^T fragments come from a row-major V tile through
//    ds_read_b64_tr_b16 (hardware transpose read).
//  * K/V tiles travel HBM -> LDS by LDS-DMA (buffer_load ... lds), double buffered; both tiles use
//    the one 256-B-row XOR image that is conflict-free for row reads and transposed reads
//    (off(row,ch) = 256 row + 16 (ch ^ ((row&3)<<2 | (row>>2)&3))), applied on the DMA source side.
//  * q/k/v are read in place from the projection output ([S, ld] rows, head h at column h*128):
//    no head-major re-layout pass exists anywhere on the path.
//  * the score-bound joint form (pre-scaled q, TdAttnParams::score_bound) has no row maximum to keep on a lane, and runs the same
//    structure on v_mfma_f32_16x16x32_bf16 (template switch M16; the tile body, its layouts and V's own LDS image: attention_common.h).
#include "attention_common.h"

// Normalise and store this wave's rows of an item: lane holds O[q][db*32 + (r&3) + 8 (r>>2) + 4 h5].  The int8 form (p.q8; compiled in
// under Q8 only: it exists for the joint attention), else 16-byte stores unless the rows are not 16-byte multiples or variant bit 0x200 asks
// for the narrow form.  Ob: the output of this item's batch entry / segment, Sq its row count.
template <bool Q8>
__device__ __forceinline__ void attn_store_item(const TdAttnParams& p, const f32x16_t (&o)[4], const float inv, bf16_t* Ob, const int Sq,
                                                const int head, const int q, const int h5) {
  if constexpr (Q8) {
    if (p.q8) {
      const int qr = min(q, Sq - 1);
      attn_store_rows_q8(o, inv, p.q8 + (size_t)qr * p.ldq8 + head * D, h5, p.q8_inv[qr], p.q8_amax + qr, q < Sq);
      return;
    }
  }
  attn_store_rows(o, inv, Ob + (size_t)min(q, Sq - 1) * p.ldo + head * D, h5, (p.ldo & 7) == 0 && !(p.variant & 0x200), q < Sq);
}

// ---------------------------------------------------------------------------------------------
// One workgroup per (256-row query tile, head, batch).  Lean instruction stream: rocprofv3 PMC on the first form of this
// kernel (S=4289, 24 heads) showed 7.2 VALU instructions per MFMA and the SIMD's issue slots, not the matrix pipe (50 % busy),
// setting the pace -- two thirds of that VALU work was LDS address arithmetic (XOR-swizzled addresses recomputed per read) and
// accumulator zeroing.  Here every per-lane LDS address lives in a register for the whole kernel (8 for the K row reads,
// 8 for the V transposed reads; k-block / k-step / tile-slot parts are instruction immediates).
// ---------------------------------------------------------------------------------------------
// KVSEG (with CAUSAL and VARLEN): the packed query segments run over key ranges of their own (TdAttnParams::kv_seg_row0 / kv_seg_lens) -- context
// attention, prompts continued behind cached prefixes.  Everything it changes sits behind `if constexpr (KVSEG)`.
// M16 (with PRE, RS and FIXED, joint attention only): the tile body on the 16x16x32 MFMA (attention_common.h); V's LDS image then has its own XOR.
template <bool CAUSAL, int NWAVES, bool BIAS = false, bool VARLEN = false, bool PRE = false, bool RS = true, bool FIXED = false, bool KVSEG = false, bool M16 = false>
__global__ __launch_bounds__(NWAVES * 64, 2) void td_attn_fwd_d128_lean_kernel(const TdAttnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [K slot 0 | K slot 1 | V slot 0 | V slot 1]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h5 = lane >> 5;
  const int l31 = lane & 31;

  const int qblk = blockIdx.x;
  const int head = blockIdx.y;
  const int batch = blockIdx.z;
  const int kvhead = head / p.q_per_kv;
  const int q0 = qblk * (NWAVES * Q_WAVE) + wid * Q_WAVE;

  const bf16_t* Qb = p.Q + (size_t)batch * p.q_bstride;
  const bf16_t* Kb = p.K + (size_t)batch * p.kv_bstride;
  const bf16_t* Vb = p.V + (size_t)batch * p.kv_bstride;
  bf16_t* Ob = p.O + (size_t)batch * p.o_bstride;
  int Sq = p.Sq, Skv = p.Skv, c_off = p.causal_offset;
  if constexpr (VARLEN) {
    // packed segments (the vision towers' cu_seqlens): segment `batch` = rows [seg_starts[b], seg_starts[b+1]) of q, k, v and o,
    // full attention inside it; the grid is sized for the longest segment, workgroups past this one's rows leave at once
    const int r0 = p.seg_starts[batch];
    Sq = Skv = p.seg_starts[batch + 1] - r0;
    if (qblk * (NWAVES * Q_WAVE) >= Sq) return;
    if constexpr (KVSEG) {
      // ... its keys are rows [kv_seg_row0[b], + kv_seg_lens[b]) of K / V: the base pointers and, below, the descriptors are the segment's own, so a
      // neighbouring slot's rows are out of range, not merely masked.  Device values are clamped, never trusted: fewer keys than queries count as Sq
      const int k0 = max(p.kv_seg_row0[batch], 0);
      Skv = max(p.kv_seg_lens[batch], Sq);
      c_off = Skv - Sq;
      Qb += (size_t)r0 * p.ldq; Kb += (size_t)k0 * p.ldkv; Vb += (size_t)k0 * p.ldkv; Ob += (size_t)r0 * p.ldo;
    } else {
      Qb += (size_t)r0 * p.ldq; Kb += (size_t)r0 * p.ldkv; Vb += (size_t)r0 * p.ldkv; Ob += (size_t)r0 * p.ldo;
    }
  }

  const unsigned q_bytes = (unsigned)(((long long)(Sq - 1) * p.ldq + p.Hq * D) * 2);
  // batched KV-cached decode: sequence `batch` has its own cache length (causal instantiation only, so the joint-attention
  // instruction stream of FLUX is untouched); keys visible to query row q: key <= q + (Skv - Sq)
  if constexpr (CAUSAL) {
    if (p.kv_lens) { Skv = p.kv_lens[batch]; c_off = Skv - p.Sq; }
  }
  const unsigned kv_bytes = (unsigned)(((long long)(Skv - 1) * p.ldkv + p.Hkv * D) * 2);
  __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)Qb, 0, q_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, kv_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, kv_bytes, 0x00020000);

  int nt = (Skv + KV_TILE - 1) / KV_TILE;
  if (CAUSAL) {
    const int last_q = min(Sq, (qblk + 1) * NWAVES * Q_WAVE) - 1 + c_off;
    nt = min(nt, last_q / KV_TILE + 1);
  }

  constexpr int GROUPS = KV_TILE / 4;
  constexpr int SG = (GROUPS + NWAVES - 1) / NWAVES;
  const int srow = lane >> 4;
  unsigned voffK[SG], voffV[SG];
#pragma unroll
  for (int s = 0; s < SG; ++s) {
    const int g = wid + NWAVES * s;
    const int swz = (srow << 2) | (g & 3);
    const int chunk = (lane & 15) ^ swz;
    voffK[s] = (unsigned)(g * 4 + srow) * (unsigned)p.ldkv * 2u + (unsigned)(kvhead * D + chunk * 8) * 2u;
    voffV[s] = M16 ? (unsigned)(g * 4 + srow) * (unsigned)p.ldkv * 2u + (unsigned)(kvhead * D + attn16_v_src_chunk(g, lane) * 8) * 2u : voffK[s];
  }
  auto stage = [&](int slot, int t) {
    const unsigned tile_off = (unsigned)t * KV_TILE * (unsigned)p.ldkv * 2u;
#pragma unroll
    for (int s = 0; s < SG; ++s) {
      const int g = wid + NWAVES * s;
      if (GROUPS % NWAVES == 0 || g < GROUPS) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, (TD_LDS void*)(smem + slot * TILE_BYTES + g * 1024), 16, voffK[s] + tile_off, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (TD_LDS void*)(smem + (2 + slot) * TILE_BYTES + g * 1024), 16, voffV[s] + tile_off, 0, 0, 0);
      }
    }
  };
  stage(0, 0);

  if constexpr (M16) {      // the whole item on the 16x16x32 body
    static_assert(!CAUSAL && !BIAS && !VARLEN && PRE && RS && FIXED, "the 16x16x32 body serves the score-bound joint form only");
    bf16x8_t qf[2][4];
    attn16_load_q(qf, rsQ, q0, head, p.ldq, lane);
    unsigned ka[4], va[8];
    attn16_lds_addrs((unsigned)(uintptr_t)(TD_LDS char*)smem, lane, ka, va);
    f32x4_t o[8][2], ls[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) o[dt][0][i] = o[dt][1][i] = 0.f;
      ls[0][i] = ls[1][i] = 0.f;
    }
    attn16_run_tiles(o, ls, qf, ka, va, 0, nt, Skv, lane, stage);
    const float l[2] = {ls[0][0], ls[1][0]};
    attn16_store_rows(o, l, Ob + head * D, p.ldo, q0, Sq, lane, (p.ldo & 7) == 0 && !(p.variant & 0x200));
    return;
  }

  bf16x8_t qf[8];
  {
    const unsigned qoff = (unsigned)(q0 + l31) * (unsigned)p.ldq * 2u + (unsigned)(head * D + 8 * h5) * 2u;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsQ, qoff + ks * 32, 0, 0);
      qf[ks] = __builtin_bit_cast(bf16x8_t, v);
    }
  }

  // ---- resident per-lane LDS byte addresses of slot 0 (the other slot is an immediate offset in the tile body) ----
  const unsigned lds0 = (unsigned)(uintptr_t)(TD_LDS char*)smem;   // LDS byte address of the tile area
  unsigned ka[8];      // K row read: row l31 (+32 kb as an immediate), chunk (2 ks + h5) ^ swz(row)
  {
    const unsigned ksw = ((lane & 3) << 2) | ((lane >> 2) & 3);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) ka[ks] = lds0 + l31 * 256 + (((2 * ks + h5) ^ ksw) << 4);
  }
  unsigned va[2][4];   // V transposed read [jj][db]: row 4 h5 + vq + 8 jj (+32 kb + 16 s as immediates)
  {
    const unsigned vq = (lane & 15) >> 2, vp = lane & 3;
    const unsigned vchunk = 2 * ((lane >> 4) & 1) + (vp >> 1);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const unsigned swz = (vq << 2) | ((2 * jj + h5) & 3);   // ((row&3)<<2) | ((row>>2)&3), independent of kb, s
#pragma unroll
      for (int db = 0; db < 4; ++db)
        va[jj][db] = lds0 + 2 * TILE_BYTES + (4 * h5 + vq + 8 * jj) * 256 + (((4 * db + vchunk) ^ swz) << 4) + 8 * (vp & 1);
    }
  }

  f32x16_t o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  if ((p.variant & 0x100) && wid >= 4) __builtin_amdgcn_s_setprio(1);   // static priority for the younger half (A/B switch)
  f32x16_t lacc;                      // row sums: every register holds the whole sum of its lane's query row
#pragma unroll
  for (int r = 0; r < 16; ++r) lacc[r] = 0.f;
  float m_run = 0.f;                  // reference point of the row's exponentials (bf16-representable; set by the first tile)
  const bf16x8_t kone = {(short)(h5 == 0 ? 0x3F80 : 0), 0, 0, 0, 0, 0, 0, 0};   // K-side fragment of the reference k-step: column 0 = 1
  bf16x8_t qnegm = {0, 0, 0, 0, 0, 0, 0, 0};                                       // Q-side: row 0 = -m_run

  const float c = p.scale * 1.4426950408889634f;
  const int q_pos = q0 + l31 + c_off;

  // The tile body is instantiated for both double-buffer slots: the slot offset of every LDS read is then an instruction
  // immediate instead of 16 address flips (v_xor) per tile and wave.
  auto tile = [&](const int t, auto slot_tag) {
    constexpr unsigned PO = decltype(slot_tag)::value * TILE_BYTES;
    // tile t landed (MY pieces: the explicit vmcnt -- a workgroup-scope fence orders LDS traffic with lgkmcnt only, and LDS-DMA
    // completes on vmcnt; the compiler used to wait by accident, in front of its transposed-read builtin) and, behind the barrier,
    // everyone's; slot (t+1)&1 no longer read
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < nt) stage((t + 1) & 1, t + 1);

    f32x16_t st[2];
    attn_tile_scores<PO, FIXED>(st, qf, kone, qnegm, ka);      // S^T - m = K . Q^T - 1 . m

    const int key0 = t * KV_TILE;
    if constexpr (BIAS) {   // additive score bias in the scaled domain: (s + bias/scale) * scale = s*scale + bias
      const float inv_scale = 1.0f / p.scale;
      const int qrow = min(q0 + l31, p.Sq - 1);
      const float* bp = p.bias + ((size_t)head * p.Sq + qrow) * p.Skv + key0 + 4 * h5;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int kbase = key0 + kb * 32 + 8 * g4 + 4 * h5;
          if (kbase + 4 <= p.Skv) {
            const f32x4_t bv = *(const f32x4_t*)(bp + kb * 32 + 8 * g4);
#pragma unroll
            for (int r = 0; r < 4; ++r) st[kb][4 * g4 + r] += bv[r] * inv_scale;
          }
        }
    }
    const bool need_mask = (key0 + KV_TILE > Skv) || (CAUSAL && key0 + KV_TILE - 1 > q0 + c_off);
    if (need_mask) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h5;
          if ((key >= Skv) || (CAUSAL && key > q_pos)) st[kb][r] = -INFINITY;
        }
    }

    attn_tile_softmax_pv<PO, PRE, RS, FIXED>(st, o, lacc, m_run, qnegm, t == 0, c, va, h5);
  };
  {
    int t = 0;
    for (; t + 1 < nt; t += 2) {
      tile(t, std::integral_constant<unsigned, 0>{});
      tile(t + 1, std::integral_constant<unsigned, 1>{});
    }
    if (t < nt) tile(t, std::integral_constant<unsigned, 0>{});
  }

  const float inv = 1.0f / (RS ? lacc[0] : half_swap_sum(lacc[0]));
  // (the int8 output form exists for the joint attention only: it stays out of the other streams)
  attn_store_item<!CAUSAL && !BIAS && !VARLEN>(p, o, inv, Ob, Sq, head, q0 + l31, h5);
#endif
}


// ---------------------------------------------------------------------------------------------
// Stream-K form of the kernel above for joint (non-causal) attention: the launch is ONE round of persistent workgroups.
//
// FLUX at 1024^2: 17 query tiles x 24 heads = 408 workgroups of 68 KV tiles each on 256 CUs -- two rounds, the second 59 %
// empty.  Here the 408 x 68 (item, KV tile) iterations are cut into G equal contiguous ranges, one per workgroup, G = number
// of CUs.  A range starts inside an item and ends inside another, so a workgroup runs
//   [tail part of item a : KV tiles kb..nt) ] [whole items ...] [head part of item z : KV tiles 0..ke) ]
// and every item is split over at most two workgroups (a range is longer than an item).  The two owners of a split item
// combine their un-normalised online-softmax states (O accumulators, row max, row sum: 68 floats per lane) exactly as two KV
// tiles are combined inside the loop, and whoever arrives SECOND does it -- nobody ever waits:
//   * the owner of the TAIL part (it meets the item first thing in its life) writes its state to slot T[j] of the boundary j
//     between the two ranges and draws a ticket from cnt[j]; ticket 0: done, ticket 1: the other side has already left its
//     state in H[j] -- read it, combine, normalise, store;
//   * the owner of the HEAD part (it meets the item last) first looks at cnt[j]: 1 (the normal case) -- read T[j], combine with
//     the state it holds in registers, normalise, store; 0 -- leave its own state in H[j] and draw a ticket, and if that comes
//     back 1 after all, finish as above from registers.
// With no wait there is no forward-progress assumption: any number of these launches may share the chip with anything else,
// in any dispatch order (a spin version deadlocks when a consumer's producer is not resident).  The hand-off is the
// placement-independent recipe of the guide (6, Guideline 16 R1 with a counter as the flag): write-through (sc1) 16-byte
// stores, every storing wave drains (s_waitcnt vmcnt(0)), workgroup barrier, ONE agent-scope atomic add; the reader's side is
// ONE agent-scope acquire after the atomic that told it, s_waitcnt, barrier, plain loads.  The finisher zeroes cnt[j]; the
// workspace (one per engine context / stream: concurrent launches must not share it) is zeroed when it is created.
// ---------------------------------------------------------------------------------------------

template <int NWAVES, bool XCD_REMAP, bool PRE = false, bool RS = true, bool FIXED = false, bool M16 = false>
__global__ __launch_bounds__(NWAVES * 64, 2) void td_attn_fwd_d128_streamk_kernel(const TdAttnParams p, char* __restrict__ ws,
                                                                                  const int n_qblk, const int nt) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [K slot 0 | K slot 1 | V slot 0 | V slot 1 | ticket word]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h5 = lane >> 5;
  const int l31 = lane & 31;
  TD_LDS unsigned* const ticket_lds = (TD_LDS unsigned*)(smem + 4 * TILE_BYTES);

  const int G = gridDim.x;
  long long it, it_end;
  const int r = attn_sk_range<XCD_REMAP>((long long)n_qblk * p.Hq * p.batch * nt, it, it_end);

  const int Skv = p.Skv;
  constexpr int GROUPS = KV_TILE / 4;
  constexpr int SG = (GROUPS + NWAVES - 1) / NWAVES;
  const int srow = lane >> 4;
  const float c = p.scale * 1.4426950408889634f;
  const float cc = PRE ? 1.0f : c;          // scale of the stored reference points: log2 units when q arrives pre-scaled
  const bf16x8_t kone = {(short)(h5 == 0 ? 0x3F80 : 0), 0, 0, 0, 0, 0, 0, 0};   // K-side fragment of the reference k-step (attn_tile_scores)

  // ---- resident per-lane LDS byte addresses of slot 0 (the other slot is an immediate offset in the tile body) ----
  const unsigned lds0 = (unsigned)(uintptr_t)(TD_LDS char*)smem;
  unsigned ka[8];
  {
    const unsigned ksw = ((lane & 3) << 2) | ((lane >> 2) & 3);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) ka[ks] = lds0 + l31 * 256 + (((2 * ks + h5) ^ ksw) << 4);
  }
  unsigned va[2][4];
  {
    const unsigned vq = (lane & 15) >> 2, vp = lane & 3;
    const unsigned vchunk = 2 * ((lane >> 4) & 1) + (vp >> 1);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const unsigned swz = (vq << 2) | ((2 * jj + h5) & 3);
#pragma unroll
      for (int db = 0; db < 4; ++db)
        va[jj][db] = lds0 + 2 * TILE_BYTES + (4 * h5 + vq + 8 * jj) * 256 + (((4 * db + vchunk) ^ swz) << 4) + 8 * (vp & 1);
    }
  }

  unsigned ka16[4], va16[8];      // M16: the 16x16x32 body's addresses (attention_common.h)
  if constexpr (M16) attn16_lds_addrs(lds0, lane, ka16, va16);

  if ((p.variant & 0x100) && wid >= 4) __builtin_amdgcn_s_setprio(1);   // static priority for the younger half (A/B switch)
  while (it < it_end) {
    // ---- the part of an item this workgroup runs now: KV tiles [kb, ke) of item `item` -------------------------------
    const int item = (int)(it / nt);
    const int kb = (int)(it - (long long)item * nt);
    const int ke = (int)min((long long)nt, kb + (it_end - it));
    __builtin_assume(ke > kb);       // a part is never empty
    it += ke - kb;
    const int qblk = item % n_qblk;
    const int hb = item / n_qblk;
    const int head = hb % p.Hq, batch = hb / p.Hq;
    const int kvhead = head / p.q_per_kv;
    const int q0 = qblk * (NWAVES * Q_WAVE) + wid * Q_WAVE;

    const bf16_t* Qb = p.Q + (size_t)batch * p.q_bstride;
    const bf16_t* Kb = p.K + (size_t)batch * p.kv_bstride;
    const bf16_t* Vb = p.V + (size_t)batch * p.kv_bstride;
    const unsigned q_bytes = (unsigned)(((long long)(p.Sq - 1) * p.ldq + p.Hq * D) * 2);
    const unsigned kv_bytes = (unsigned)(((long long)(Skv - 1) * p.ldkv + p.Hkv * D) * 2);
    __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)Qb, 0, q_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, kv_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, kv_bytes, 0x00020000);

    unsigned voffK[SG], voffV[SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) {
      const int g = wid + NWAVES * s;
      const int swz = (srow << 2) | (g & 3);
      const int chunk = (lane & 15) ^ swz;
      voffK[s] = (unsigned)(g * 4 + srow) * (unsigned)p.ldkv * 2u + (unsigned)(kvhead * D + chunk * 8) * 2u;
      voffV[s] = M16 ? (unsigned)(g * 4 + srow) * (unsigned)p.ldkv * 2u + (unsigned)(kvhead * D + attn16_v_src_chunk(g, lane) * 8) * 2u : voffK[s];
    }
    auto stage = [&](int slot, int t) {
      const unsigned tile_off = (unsigned)t * KV_TILE * (unsigned)p.ldkv * 2u;
#pragma unroll
      for (int s = 0; s < SG; ++s) {
        const int g = wid + NWAVES * s;
        if (GROUPS % NWAVES == 0 || g < GROUPS) {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, (TD_LDS void*)(smem + slot * TILE_BYTES + g * 1024), 16, voffK[s] + tile_off, 0, 0, 0);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (TD_LDS void*)(smem + (2 + slot) * TILE_BYTES + g * 1024), 16, voffV[s] + tile_off, 0, 0, 0);
        }
      }
    };
    __syncthreads();          // the previous part's last tile is no longer read by any wave
    stage(0, kb);

    if constexpr (M16) {      // this part of the item on the 16x16x32 body
      static_assert(PRE && RS && FIXED, "the 16x16x32 body serves the score-bound form only");
      bf16x8_t qf[2][4];
      attn16_load_q(qf, rsQ, q0, head, p.ldq, lane);
      f32x4_t o[8][2], ls[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[dt][0][i] = o[dt][1][i] = 0.f;
        ls[0][i] = ls[1][i] = 0.f;
      }
      attn16_run_tiles(o, ls, qf, ka16, va16, kb, ke, Skv, lane, stage);
      float l[2] = {ls[0][0], ls[1][0]};
      if (kb > 0 || ke < nt) {      // the hand-off state: the 64 accumulator registers in the order n = 8 dt + 4 qb + i, and the two row sums
        f32x16_t o16[4];
#pragma unroll
        for (int n = 0; n < 64; ++n) o16[n >> 4][n & 15] = o[n >> 3][(n >> 2) & 1][n & 3];
        if (!attn_sk_handoff<true>(o16, l[1], l[0], 1.0f, r, G, kb > 0, ws, ticket_lds, tid, wid)) continue;
#pragma unroll
        for (int n = 0; n < 64; ++n) o[n >> 3][(n >> 2) & 1][n & 3] = o16[n >> 4][n & 15];
      }
      attn16_store_rows(o, l, p.O + (size_t)batch * p.o_bstride + head * D, p.ldo, q0, p.Sq, lane, (p.ldo & 7) == 0 && !(p.variant & 0x200));
      continue;
    }

    bf16x8_t qf[8];
    {
      const unsigned qoff = (unsigned)(q0 + l31) * (unsigned)p.ldq * 2u + (unsigned)(head * D + 8 * h5) * 2u;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsQ, qoff + ks * 32, 0, 0);
        qf[ks] = __builtin_bit_cast(bf16x8_t, v);
      }
    }

    f32x16_t o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) o[db][rr] = 0.f;
    f32x16_t lacc;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) lacc[rr] = 0.f;
    float m_run = 0.f;
    bf16x8_t qnegm = {0, 0, 0, 0, 0, 0, 0, 0};
    auto tile = [&](const int t, auto slot_tag) {
      constexpr unsigned SLOT = decltype(slot_tag)::value;
      constexpr unsigned PO = SLOT * TILE_BYTES;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my pieces of tile t landed (explicit: see the plain-grid kernel) ...
      __syncthreads();                                        // ... and everyone's; the other slot is no longer read
      if (t + 1 < ke) stage(SLOT ^ 1, t + 1);

      f32x16_t st[2];
      attn_tile_scores<PO, FIXED>(st, qf, kone, qnegm, ka);

      const int key0 = t * KV_TILE;
      if (key0 + KV_TILE > Skv) {        // last tile: keys >= Skv are masked
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int rr = 0; rr < 16; ++rr) {
            const int key = key0 + kk * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * h5;
            if (key >= Skv) st[kk][rr] = -INFINITY;
          }
      }

      attn_tile_softmax_pv<PO, PRE, RS, FIXED>(st, o, lacc, m_run, qnegm, t == kb, c, va, h5);
    };
    {
      int t = kb;
      for (; t + 1 < ke; t += 2) {
        tile(t, std::integral_constant<unsigned, 0>{});
        tile(t + 1, std::integral_constant<unsigned, 1>{});
      }
      if (t < ke) tile(t, std::integral_constant<unsigned, 0>{});
    }
    float l_run = RS ? lacc[0] : half_swap_sum(lacc[0]);           // the complete row sum (RS: every register of lacc holds it, in both lane halves)
    // ---- what happens to the state: leave it for the other owner, combine with the other owner's, or just finish ----------
    if ((kb > 0 || ke < nt) && !attn_sk_handoff(o, m_run, l_run, cc, r, G, kb > 0, ws, ticket_lds, tid, wid)) continue;

    attn_store_item<true>(p, o, 1.0f / l_run, p.O + (size_t)batch * p.o_bstride, p.Sq, head, q0 + l31, h5);
  }
#endif
}

namespace {

size_t sk_ws_bytes(int ranges) { return (size_t)SK_HEADER_BYTES + (size_t)2 * ranges * SK_SLOT_FLOATS * sizeof(float); }

// Workspaces for callers that bring none (the plain C entry point): one per (device, stream), created on the first launch
// that needs it -- call td_attention_bf16 once per stream before capturing it into a hipGraph.  Concurrent launches must
// not share a workspace, and launches on one stream never overlap.
int sk_pooled_workspace(int dev, int ranges, hipStream_t stream, char** out) {
  struct Entry { int dev; hipStream_t stream; int ranges; char* ws; };
  static std::mutex mu;
  static std::vector<Entry> pool;
  std::lock_guard<std::mutex> lock(mu);
  for (auto& e : pool)
    if (e.dev == dev && e.stream == stream && e.ranges >= ranges) { *out = e.ws; return 0; }
  char* w = nullptr;
  TD_CHECK_HIP(hipMalloc((void**)&w, sk_ws_bytes(ranges)));
  // zeroed ON the launching stream: a null-stream memset is not ordered with a non-blocking stream, and the first persistent
  // launch of a new stream would race it for the hand-off counters
  TD_CHECK_HIP(hipMemsetAsync(w, 0, SK_HEADER_BYTES, stream));
  pool.push_back(Entry{dev, stream, ranges, w});
  *out = w;
  return 0;
}

int device_cus(int dev) {
  static std::atomic<int> cus[64] = {};
  int n = cus[dev & 63].load(std::memory_order_relaxed);
  if (n == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    n = prop.multiProcessorCount;
    cus[dev & 63].store(n, std::memory_order_relaxed);
  }
  return n;
}

}  // namespace

// shared with attention_fp8.hip
int td_attn_device_cus(int dev) { return device_cus(dev); }
int td_attn_pooled_workspace(int dev, int ranges, hipStream_t stream, char** out) { return sk_pooled_workspace(dev, ranges, stream, out); }

int td_attn_launch(const TdAttnParams& p, hipStream_t stream) {
  TD_CHECK_ARG(p.head_dim == D, "td_attention: head_dim=%d unsupported (only 128)", p.head_dim);
  TD_CHECK_ARG(p.Sq > 0 && p.Skv > 0 && p.Hq > 0 && p.Hkv > 0 && p.batch > 0, "td_attention: empty problem");
  TD_CHECK_ARG(p.Hq % p.Hkv == 0, "td_attention: Hq=%d not a multiple of Hkv=%d", p.Hq, p.Hkv);
  TD_CHECK_ARG(p.ldq % 8 == 0 && p.ldkv % 8 == 0 && p.ldo % 4 == 0, "td_attention: row strides must be 16-byte multiples");
  TD_CHECK_ARG(((long long)(p.Sq + 256) * p.ldq) * 2 < (1ll << 32) && ((long long)(p.Skv + 64) * p.ldkv) * 2 < (1ll << 32),
               "td_attention: per-batch operand exceeds the 4 GiB buffer-descriptor range");
  TD_CHECK_ARG(((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V | (uintptr_t)p.O) % 16 == 0, "td_attention: pointers must be 16-byte aligned");
  if (p.kv_seg_row0 || p.kv_seg_lens) {   // packed query segments over key ranges of their own: one form, refused here, before the first HIP call
    TD_CHECK_ARG(p.kv_seg_row0 && p.kv_seg_lens && p.seg_starts,
                 "td_attention(prefix segments): kv_seg_row0 and kv_seg_lens are given together, and with seg_starts (kv_seg_row0 %s, kv_seg_lens %s, seg_starts %s)",
                 p.kv_seg_row0 ? "set" : "null", p.kv_seg_lens ? "set" : "null", p.seg_starts ? "set" : "null");
    TD_CHECK_ARG(p.causal && !p.bias && !p.kv_lens && !p.q_prescaled && !p.q8 && !p.K8,
                 "td_attention(prefix segments): causal bf16 attention only (causal=%d; no bias%s, kv_lens%s, pre-scaled q%s, int8 output%s or e4m3 cache%s)", p.causal,
                 p.bias ? " [given]" : "", p.kv_lens ? " [given]" : "", p.q_prescaled ? " [given]" : "", p.q8 ? " [given]" : "", p.K8 ? " [given]" : "");
  }
  if (p.K8) {      // an e4m3 KV cache (TdAttnParams::K8): the decode kernel's 8-bit form, there is no tile kernel that reads it
    TD_CHECK_ARG(p.Sq == 1 && p.causal && !p.bias && !p.seg_starts && (p.kv_lens || p.causal_offset == p.Skv - 1),
                 "td_attention: an e4m3 KV cache is read by the decode form only (Sq = 1, causal, no bias, no packed segments)");
    return td_attn_decode_launch(p, stream);
  }
  // one query token per sequence against its KV cache: the dedicated decode kernel (keys split over lanes, GQA group shares K/V).  Never a packed
  // launch: the decode kernel knows no seg_starts (it steps by the batch strides, which a packed launch leaves 0), so packed one-row segments
  // (max_len = 1: a pass of one-token prompts) stay on the tile kernel below
  if (p.Sq == 1 && p.causal && !p.bias && !p.seg_starts && (p.variant & 0xff) == 0 && (p.kv_lens || p.causal_offset == p.Skv - 1))
    return td_attn_decode_launch(p, stream);
  TdAttnParams q = p;
  q.q_per_kv = p.Hq / p.Hkv;
  // Structures that lost the in-process A/B on MI355X and were removed: a 4-wave workgroup with ONE wave per SIMD, each wave
  // owning two 32-row blocks half a tile apart (softmax of one block on the VALU under the other block's MFMAs, 3-deep K / V
  // rings, the guide's "512-register" shape; round 3: correct, 448 vs 219 us -- with > 256 live registers hipcc puts every
  // accumulator AND the Q fragments in AGPRs and moves ~400 values per tile through v_accvgpr_read/write, plus 1 KB of scratch),
  // ping-pong wave halves with a 3-deep V ring (-9 %),
  // 4-wave workgroups two per CU (-35 %), intra-wave QK^T(t+1) / softmax(t) software pipelining (-6 %), the first
  // lockstep kernel with per-read address arithmetic (-15 %).
  constexpr int NW = 8;
  constexpr int lds = 4 * TILE_BYTES;
  int dev = 0;
  TD_CHECK_HIP(hipGetDevice(&dev));
  dim3 grid((p.Sq + NW * Q_WAVE - 1) / (NW * Q_WAVE), p.Hq, p.batch);
  if (p.bias) TD_CHECK_ARG(p.Skv % 4 == 0 && ((uintptr_t)p.bias) % 16 == 0 && p.batch == 1, "td_attention: bias needs Skv %% 4 == 0, 16-byte alignment, batch 1");
  if (p.kv_lens) TD_CHECK_ARG(p.causal && !p.bias, "td_attention: per-sequence kv lengths exist for the causal kernel only");
  if (p.q_prescaled) TD_CHECK_ARG(!p.causal && !p.bias && !p.kv_lens && !p.seg_starts, "td_attention: pre-scaled q is a form of the joint (unmasked) attention only");
  TD_CHECK_ARG(p.score_bound >= 0.f && p.score_bound <= 48.f && (p.score_bound == 0.f || p.q_prescaled), "td_attention: a score bound goes with pre-scaled q (joint attention) and lies in (0, 48] octaves (0 = none)");
  if (p.q8) TD_CHECK_ARG(!p.causal && !p.bias && !p.kv_lens && !p.seg_starts && p.batch == 1 && p.q8_inv && p.q8_amax && p.ldq8 % 8 == 0 && ((uintptr_t)p.q8) % 8 == 0,
                         "td_attention: the int8 output form is for the joint attention of one batch entry, with 8-byte aligned rows");
  if (p.seg_starts && p.kv_seg_row0) {   // ... with their own key ranges (checked on entry): Sq sizes the grid, Skv only the descriptor check above
    if (int e = attn_launch<td_attn_fwd_d128_lean_kernel<true, NW, false, true, false, true, false, true>>(grid, NW * 64, lds, stream, dev, q)) return e;
    TD_CHECK_LAUNCH();
    return 0;
  }
  if (p.seg_starts) {   // packed segments: plain grid over (query tiles of the longest segment, heads, segments)
    TD_CHECK_ARG(!p.bias && !p.kv_lens && p.Sq == p.Skv && (!p.causal || p.causal_offset == 0),
                 "td_attention(varlen): full or causal (offset 0) attention inside each segment only (no bias or cache lengths)");
    // causal: the packed prefill of the Qwen2-VL engine (prompts of different lengths back to back, no padding rows)
    if (int e = p.causal ? attn_launch<td_attn_fwd_d128_lean_kernel<true, NW, false, true>>(grid, NW * 64, lds, stream, dev, q)
                         : attn_launch<td_attn_fwd_d128_lean_kernel<false, NW, false, true>>(grid, NW * 64, lds, stream, dev, q)) return e;
    TD_CHECK_LAUNCH();
    return 0;
  }

  // joint attention with more workgroups than CUs: one round of persistent workgroups over equal (item, KV tile) ranges.
  // variant 1 = the one-workgroup-per-item kernel for every shape (in-process A/B); variant 2 = stream-K without the XCD remap.
  const int n_items = (int)(grid.x * grid.y * grid.z);
  const int cus = device_cus(dev);
  const int nt = (p.Skv + KV_TILE - 1) / KV_TILE;
  // The score-bound form runs its tile body on the 16x16x32 MFMA (attention_common.h).  Not with the int8 output: that store form is written for the
  // 32x32 register layout only; variant bit M16_FORCE_32 keeps the 32x32 body for the in-process A/B.
  const bool m16 = !p.q8 && !(p.variant & M16_FORCE_32);
  int e;
  if (!p.causal && !p.bias && !p.kv_lens && (p.variant & 0xff) != 1 && cus > 0 && n_items > cus && cus < SK_MAX_RANGES && (long long)n_items * nt < (1ll << 31)) {
    char* ws = (char*)p.sk_ws;
    if (!ws) {
      if (int rc = sk_pooled_workspace(dev, cus, stream, &ws)) return rc;
    }
    constexpr int lds_sk = lds + 16;        // + the ticket word
    const dim3 ranges(cus);
    const int n_qblk = (int)grid.x;
    if (p.q_prescaled && p.score_bound > 0.f && m16) e = attn_launch<td_attn_fwd_d128_streamk_kernel<NW, true, true, true, true, true>>(ranges, NW * 64, lds_sk, stream, dev, q, ws, n_qblk, nt);
    else if (p.q_prescaled && p.score_bound > 0.f) e = attn_launch<td_attn_fwd_d128_streamk_kernel<NW, true, true, true, true>>(ranges, NW * 64, lds_sk, stream, dev, q, ws, n_qblk, nt);
    else if (p.q_prescaled) e = attn_launch<td_attn_fwd_d128_streamk_kernel<NW, true, true>>(ranges, NW * 64, lds_sk, stream, dev, q, ws, n_qblk, nt);
    else if ((p.variant & 0xff) == 2) e = attn_launch<td_attn_fwd_d128_streamk_kernel<NW, false>>(ranges, NW * 64, lds_sk, stream, dev, q, ws, n_qblk, nt);
    else e = attn_launch<td_attn_fwd_d128_streamk_kernel<NW, true>>(ranges, NW * 64, lds_sk, stream, dev, q, ws, n_qblk, nt);
  } else if (p.bias) {   // separate instantiations: the score-bias loads must not touch the hot no-bias instruction stream
    e = p.causal ? attn_launch<td_attn_fwd_d128_lean_kernel<true, NW, true>>(grid, NW * 64, lds, stream, dev, q)
                 : attn_launch<td_attn_fwd_d128_lean_kernel<false, NW, true>>(grid, NW * 64, lds, stream, dev, q);
  } else if (p.q_prescaled && p.score_bound > 0.f && m16) {
    e = attn_launch<td_attn_fwd_d128_lean_kernel<false, NW, false, false, true, true, true, false, true>>(grid, NW * 64, lds, stream, dev, q);
  } else if (p.q_prescaled && p.score_bound > 0.f) {
    e = attn_launch<td_attn_fwd_d128_lean_kernel<false, NW, false, false, true, true, true>>(grid, NW * 64, lds, stream, dev, q);
  } else if (p.q_prescaled) {
    e = attn_launch<td_attn_fwd_d128_lean_kernel<false, NW, false, false, true>>(grid, NW * 64, lds, stream, dev, q);
  } else {
    e = p.causal ? attn_launch<td_attn_fwd_d128_lean_kernel<true, NW>>(grid, NW * 64, lds, stream, dev, q)
                 : attn_launch<td_attn_fwd_d128_lean_kernel<false, NW>>(grid, NW * 64, lds, stream, dev, q);
  }
  if (e) return e;
  TD_CHECK_LAUNCH();
  return 0;
}

// bytes of the stream-K hand-off workspace td_attn_launch wants in TdAttnParams::sk_ws on the current device (zero-filled
// once by the owner; one per concurrently running launch, e.g. one per engine context)
size_t td_attn_streamk_ws_bytes() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  const int cus = device_cus(dev);
  return cus > 0 && cus < SK_MAX_RANGES ? sk_ws_bytes(cus) : 0;
}
