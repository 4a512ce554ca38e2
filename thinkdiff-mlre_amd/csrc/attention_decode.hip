// KV-cached decode attention (one query token per sequence) for gfx950.
//
// The prefill kernel (attention_bf16.hip) tiles 256 query rows per workgroup; with Sq = 1 it wastes 255 of them and walks the
// cache one 64-key tile at a time in a single workgroup per head (13 us for 300 keys).  Here a workgroup owns one
// (sequence, q head): its 4 waves split the keys 16 at a time -- a key row is read once by 16 lanes (16 B each, the whole
// 256-B row coalesced) -- every 16-lane key slot keeps its own
// online-softmax state and output slice in registers, and the 16 slots are merged at the end (shuffles inside a wave, LDS
// across waves).  fp32 scores / softmax / accumulation; q.k through v_dot2c_f32_bf16.
// Semantics = td_attn_launch with Sq = 1, causal, kv_lens (keys [0, kv_lens[b]) of sequence b are visible).
//
// e4m3 KV cache (td_attn_decode_kernel<G, true>, TdAttnParams::K8; include/thinkdiff_hip.h "e4m3 KV cache"): every 128-wide head vector of a cache row is
// 128 bytes in the e4m3 power-of-two format of csrc/e4m3_pow2.h, one scale per head vector.  x^ is a bf16 value exactly, so the 8-bit form is this kernel
// on a cache that holds K^ | V^: a lane fetches 8 bytes of the 128-byte line and the line's scale, and the scale goes INTO the conversion (to bf16 for k,
// to fp32 for v), never onto a rounded value.  Deviation from vLLM's kv_cache_dtype="fp8": one scale per (token, kv head, k or v) instead of
// one per tensor.  Below the kernel: td_kv_quant_rows_kernel / td_kv_dequant_rows_kernel, which move bf16 k | v rows into and out of that format (prefill
// scatter, staging of a continued forward, td_qwen2_read_kv).
#include <atomic>

#include <type_traits>

#include "td_common.h"
#include "td_kernels.h"
#include "e4m3_pow2.h"
#include "qk_rope_math.h"

namespace {

// What a lane fetches of one key: its 16 B of the bf16 k and v head rows, or -- e4m3 cache -- its 8 B of each 128-byte line and the line's two scales.
struct KeyRaw16 { u32x4_t k, v; };
struct KeyRaw8 { u32x2_t k, v; float ks, vs; };

// KV8: the cache holds e4m3 bytes with one power-of-two scale per (row, kv head, k or v) (TdAttnParams::K8).  A head row is one 128-byte line plus one
// scale; k is converted with its scale into the bf16 pairs v_dot2c takes (e4m3p2_to_bf16), v into the fp32 values the accumulation takes
// (e4m3p2_to_f32) -- both exact, so from there on the arithmetic is that of the bf16 form on the dequantised cache, instruction for instruction.
// A template parameter: the key loop has no branch on the format.
// VR ("verify rows", td_attn_verify_launch's row-per-workgroup form): blockIdx.y = vr_tmax b + r is query row r of sequence b of a multi-row step
// (TdAttnParams::vr_*): it sees len0[b] + r keys of slot vr_slot[b], its q / o row is vr_row0[b] + r, and a row past the sequence's count leaves at once.
template <int G, bool KV8, bool VR = false>
__global__ __launch_bounds__(256) void td_attn_decode_kernel(const TdAttnParams p) {
  using KeyRaw = std::conditional_t<KV8, KeyRaw8, KeyRaw16>;
  __shared__ float sm_m[4][G], sm_l[4][G];
  __shared__ float sm_o[4][G][128];
  // one workgroup per (q-head group of G, sequence); G = 1 launches one per q head: K/V of a kv head are then read by each of
  // its q heads (from L2), which is cheap next to the parallelism it buys at small batch
  const int qg = blockIdx.x;
  int b = blockIdx.y, vr_len = 0, vr_cslot = 0;      // b: the q / o row (and, without VR, the sequence)
  if constexpr (VR) {
    const int seq = b / p.vr_tmax, r = b % p.vr_tmax;
    int t = p.vr_rows[seq];
    t = t < 1 ? 1 : (t > p.vr_tmax ? p.vr_tmax : t);
    if (r >= t) return;
    vr_len = p.vr_len0[seq] + r; vr_cslot = p.vr_slot[seq]; b = p.vr_row0[seq] + r;
  }
  const int kvh = (qg * G) / p.q_per_kv;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int j = lane & 15;                       // 16-B chunk of the 256-B head row
  const int slot = wid * 4 + (lane >> 4);        // key slot 0..15
  const int len = VR ? vr_len : p.kv_lens ? p.kv_lens[b] : p.Skv;
  const int cslot = VR ? vr_cslot : p.dec_slots ? p.dec_slots[b] : b;      // the cache slot of sequence b
  const bf16_t* Kb = KV8 ? nullptr : p.K + (size_t)cslot * p.kv_bstride + (size_t)kvh * 128 + 8 * j;
  const bf16_t* Vb = KV8 ? nullptr : p.V + (size_t)cslot * p.kv_bstride + (size_t)kvh * 128 + 8 * j;
  const uint8_t* Kb8 = KV8 ? p.K8 + (size_t)cslot * p.kv_bstride + (size_t)kvh * 128 + 8 * j : nullptr;      // (ldkv / kv_bstride in bytes)
  const uint8_t* Vb8 = KV8 ? p.V8 + (size_t)cslot * p.kv_bstride + (size_t)kvh * 128 + 8 * j : nullptr;
  const float* Ksb = KV8 ? p.k_scale + (size_t)cslot * p.s_bstride + kvh : nullptr;
  const float* Vsb = KV8 ? p.v_scale + (size_t)cslot * p.s_bstride + kvh : nullptr;
  const bf16_t* Qb = p.Q + (size_t)b * p.q_bstride + (size_t)qg * G * 128 + 8 * j;
  u32x4_t q[G];
#pragma unroll
  for (int g = 0; g < G; ++g) q[g] = *(const u32x4_t*)(Qb + (size_t)g * 128);
  // fused rotary embedding + cache write (TdAttnParams::dec_kv_new): lane j of a 16-lane row holds head dims 8j .. 8j+7; rotate_half pairs dim d with
  // d +- 64, i.e. lane j with lane j ^ 8 of the same row (one DPP rotate by 8)
  const bool fused = !VR && p.dec_kv_new != nullptr;
  u32x4_t knew = {0u, 0u, 0u, 0u}, vnew = {0u, 0u, 0u, 0u};
  if (fused) {
    float cs[8], sn[8];
    {
      const f32x4_t c0 = *(const f32x4_t*)(p.dec_cos + (size_t)b * 128 + 8 * j), c1 = *(const f32x4_t*)(p.dec_cos + (size_t)b * 128 + 8 * j + 4);
      const f32x4_t s0 = *(const f32x4_t*)(p.dec_sin + (size_t)b * 128 + 8 * j), s1 = *(const f32x4_t*)(p.dec_sin + (size_t)b * 128 + 8 * j + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) { cs[i] = c0[i]; cs[4 + i] = c1[i]; sn[i] = s0[i]; sn[4 + i] = s1[i]; }
    }
    auto rope = [&](const u32x4_t raw) -> u32x4_t {
      float x[8], other[8], y[8];
      unsigned r4[4] = {raw[0], raw[1], raw[2], raw[3]};
#pragma unroll
      for (int i = 0; i < 4; ++i) { x[2 * i] = bf_lo(r4[i]); x[2 * i + 1] = bf_hi(r4[i]); }
#pragma unroll
      for (int i = 0; i < 8; ++i) other[i] = row16_xor8(x[i]);
      qk_rope_half8_rbf(x, other, j < 8, cs, sn, y);
      return u32x4_t{pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3]), pack_bf2(y[4], y[5]), pack_bf2(y[6], y[7])};
    };
#pragma unroll
    for (int g = 0; g < G; ++g) q[g] = rope(q[g]);
    const int KVW = p.Hkv * 2 * 128;
    knew = rope(*(const u32x4_t*)(p.dec_kv_new + (size_t)b * KVW + (size_t)kvh * 128 + 8 * j));
    vnew = *(const u32x4_t*)(p.dec_kv_new + (size_t)b * KVW + (size_t)(p.Hkv + kvh) * 128 + 8 * j);
    if constexpr (KV8) {
      // the new key and value are rounded through the format BEFORE use (row maximum over the 16 lanes by DPP, exponent, bytes, x^ back into the registers
      // one_key reads): this launch sees the values every later launch will read from the cache
      float ks, vs;
      const u32x2_t kb = kv8_round_row(knew, ks), vb = kv8_round_row(vnew, vs);
      if ((qg * G) % p.q_per_kv == 0 && tid < 16) {      // one 16-lane row of the kv head's first workgroup writes the new line and its scales
        const size_t row = (size_t)p.dec_row_off[b];
        *(u32x2_t*)((uint8_t*)p.K8 + row * p.ldkv + (size_t)kvh * 128 + 8 * j) = kb;
        *(u32x2_t*)((uint8_t*)p.V8 + row * p.ldkv + (size_t)kvh * 128 + 8 * j) = vb;
        if (j == 0) {
          ((float*)p.k_scale)[row * p.lds + kvh] = ks;
          ((float*)p.v_scale)[row * p.lds + kvh] = vs;
        }
      }
    } else if ((qg * G) % p.q_per_kv == 0 && tid < 16) {      // one 16-lane row of the kv head's first workgroup writes the new cache row
      bf16_t* dst = (bf16_t*)p.K + (size_t)p.dec_row_off[b] * p.ldkv;      // (a ROW index: 256 sequences x 8192 rows x 1024 elements pass 2^31)
      *(u32x4_t*)(dst + (size_t)kvh * 128 + 8 * j) = knew;
      *(u32x4_t*)(dst + (size_t)(p.Hkv + kvh) * 128 + 8 * j) = vnew;
    }
  }
  const int len_cache = fused ? len - 1 : len;      // keys that are read from the cache; with the fused form the last key sits in registers
  float m[G], l[G], o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY; l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[g][i] = 0.f;
  }
  const float sc = p.scale * 1.4426950408889634f;   // softmax in base 2
  // one key of this slot: scores of the G query heads against it, online softmax, value accumulation
  auto one_key_f = [&](const u32x4_t& kk, const float (&vf)[8]) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float s = row16_sum(dot8(kk, q[g], 0.f)) * sc;
      const float mn = fmaxf(m[g], s);
      const float corr = __builtin_amdgcn_exp2f(m[g] - mn), pe = __builtin_amdgcn_exp2f(s - mn);
      m[g] = mn;
      l[g] = l[g] * corr + pe;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[g][i] = o[g][i] * corr + pe * vf[i];
    }
  };
  auto one_key = [&](const u32x4_t& kk, const u32x4_t& vv) {
    float vf[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { vf[2 * i] = bf_lo(vv[i]); vf[2 * i + 1] = bf_hi(vv[i]); }
    one_key_f(kk, vf);
  };
  auto fetch = [&](int key) -> KeyRaw {
    if constexpr (KV8) {
      return KeyRaw8{*(const u32x2_t*)(Kb8 + (size_t)key * p.ldkv), *(const u32x2_t*)(Vb8 + (size_t)key * p.ldkv), Ksb[(size_t)key * p.lds], Vsb[(size_t)key * p.lds]};
    } else {
      return KeyRaw16{*(const u32x4_t*)(Kb + (size_t)key * p.ldkv), *(const u32x4_t*)(Vb + (size_t)key * p.ldkv)};
    }
  };
  auto use = [&](const KeyRaw& r) {
    if constexpr (KV8) {
      float vf[8];
      e4m3p2_to_f32(r.v, r.vs, vf);
      one_key_f(e4m3p2_to_bf16(r.k, r.ks), vf);
    } else {
      one_key(r.k, r.v);
    }
  };
  // The loop is a chain of dependent HBM / L2 round trips (one key row per slot and trip: ~0.6 us each, 19 trips for 300 keys = the 12 us the
  // kernel took per layer at one sequence): four keys per slot are fetched before the first is used, so a trip's latency covers four keys.
  // The keys of a slot are still visited in increasing order, so the arithmetic -- and the result -- is unchanged.
  // ... and the NEXT four are requested before the current four are used (register double buffer): with several query heads per workgroup the
  // arithmetic of a trip (~35 instructions per key and head) is as long as its fetch, and the two alternated instead of overlapping.
  constexpr int UN = G >= 6 ? 2 : 4;      // (6 / 7 heads per workgroup: two keys per buffer keep the kernel inside 256 registers, i.e. two waves per SIMD)
  int key = slot;
  if constexpr (G == 1) {      // one head per workgroup (small batches: the grid is heads x sequences): a trip is all fetch, nothing to overlap it with
    if constexpr (KV8) {       // half the bytes per key leave room for eight keys per trip (6 registers a key against 8): half as many dependent round trips on a long cache
      for (; key + 16 * 7 < len_cache; key += 16 * 8) {
        KeyRaw r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = fetch(key + 16 * u);
#pragma unroll
        for (int u = 0; u < 8; ++u) use(r[u]);
      }
    }
    for (; key + 16 * (UN - 1) < len_cache; key += 16 * UN) {
      KeyRaw r[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) r[u] = fetch(key + 16 * u);
#pragma unroll
      for (int u = 0; u < UN; ++u) use(r[u]);
    }
  } else if (key + 16 * (UN - 1) < len_cache) {
    KeyRaw r[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) r[u] = fetch(key + 16 * u);
    for (;;) {
      const int nkey = key + 16 * UN;
      const bool more = nkey + 16 * (UN - 1) < len_cache;
      KeyRaw rn[UN];
      if (more) {
#pragma unroll
        for (int u = 0; u < UN; ++u) rn[u] = fetch(nkey + 16 * u);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) use(r[u]);
      key = nkey;
      if (!more) break;
#pragma unroll
      for (int u = 0; u < UN; ++u) r[u] = rn[u];
    }
  }
  for (; key < len_cache; key += 16) use(fetch(key));
  if (fused && key == len - 1) one_key(knew, vnew);      // the slot that owns key len - 1 in the strided order: same arithmetic order as reading it from the cache
  // merge the 4 key slots of this wave (lanes 16 / 32 apart hold the same d-chunk), then the 4 waves through LDS
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const float mo = __shfl_xor(m[g], off, 64), lo = __shfl_xor(l[g], off, 64);
      const float mn = fmaxf(m[g], mo);
      const float ca = m[g] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[g] - mn);
      const float cb = mo == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mo - mn);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[g][i] = o[g][i] * ca + __shfl_xor(o[g][i], off, 64) * cb;
      l[g] = l[g] * ca + lo * cb;
      m[g] = mn;
    }
    if (lane < 16) {
      if (lane == 0) { sm_m[wid][g] = m[g]; sm_l[wid][g] = l[g]; }
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_o[wid][g][8 * j + i] = o[g][i];
    }
  }
  __syncthreads();
  // 256 threads: thread t writes output elements (g, d) for t = g' * 128 + d over ceil(G*128/256) passes
  bf16_t* Ob = p.O + (size_t)b * p.o_bstride + (size_t)qg * G * 128;
  for (int e = tid; e < G * 128; e += 256) {
    const int g = e >> 7, d = e & 127;
    float mn = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mn = fmaxf(mn, sm_m[w][g]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float c = sm_m[w][g] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sm_m[w][g] - mn);
      num += sm_o[w][g][d] * c;
      den += sm_l[w][g] * c;
    }
    Ob[e] = f2bf(den > 0.f ? num / den : 0.f);
  }
}

// Multi-row ("verify") decode attention: sequence b owns the query rows [row0[b], row0[b] + t[b]) of q / o, 1 <= t[b] <= TD_MAX_VERIFY_ROWS, and row j
// sees keys [0, len0[b] + j) of cache slot slot[b] -- the step of speculative decoding that checks t - 1 guessed tokens, whose k | v rows are already in
// the cache.  The kernel above serves this layout with one workgroup per row (dec_slots repeating a slot): a sequence's K/V are then read t times.
// Here one workgroup serves (q-head group G, sequence, row chunk of T): every fetched key is used for its G x T query rows.  Everything else is the
// kernel above: 16 key slots over 4 waves, key i in slot i % 16 and visited in increasing order, the register double buffer, one fp32 online-softmax
// state per (row, head), the same in-wave and LDS merge -- so row (b, j) gets the bits the kernel above gives one query with kv_lens = len0[b] + j.
// A key a row may not see is SKIPPED by predicate (the predicate is uniform over the 16 lanes of a key slot, so the DPP row sums stay whole); it is
// never scored as -inf, which on a still-empty state would be exp2(-inf - -inf).
// T is a bound, the true t[b] is read per workgroup: blockIdx.z = chunk c serves rows [c T, min(t, (c + 1) T)) and leaves at once when there are none,
// so any T is correct for any t and T only decides how many rows share one read of the keys (the launcher takes T >= t_max where G x T <= 8 allows).
struct TdAttnVerifyParams {
  const bf16_t* Q; bf16_t* O; const bf16_t* K; const bf16_t* V;
  const uint8_t* K8; const uint8_t* V8; const float* k_scale; const float* v_scale;
  int ldq, ldkv, ldo, lds;
  long long kv_bstride, s_bstride;
  const int *row0, *rows, *len0, *slot;
  int q_per_kv, t_max;      // t_max <= TD_MAX_VERIFY_ROWS: the grid has ceil(t_max / T) chunks, rows[b] is clamped to 1..t_max
  float scale;
};

template <int G, int T, bool KV8>
__global__ __launch_bounds__(256) void td_attn_verify_kernel(const TdAttnVerifyParams p) {
  using KeyRaw = std::conditional_t<KV8, KeyRaw8, KeyRaw16>;
  constexpr int S = G * T;      // (row, head) states of a workgroup
  __shared__ float sm_m[4][S], sm_l[4][S];
  __shared__ float sm_o[4][S][128];
  const int qg = blockIdx.x, b = blockIdx.y;
  int t = p.rows[b];
  t = t < 1 ? 1 : (t > p.t_max ? p.t_max : t);
  const int j0 = blockIdx.z * T;                 // first row of this chunk
  if (j0 >= t) return;                           // (uniform over the workgroup: nobody waits at the barrier below)
  const int tc = t - j0 < T ? t - j0 : T;        // rows of this chunk
  const int kvh = (qg * G) / p.q_per_kv;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int j = lane & 15;
  const int slot = wid * 4 + (lane >> 4);
  const int len_first = p.len0[b] + j0;          // keys the chunk's first row sees; row r of the chunk sees len_first + r
  const int len_last = len_first + tc - 1;       // ... its last row: no key at or past it is read
  const int cslot = p.slot[b];
  const size_t qrow = (size_t)p.row0[b] + j0;
  const bf16_t* Kb = KV8 ? nullptr : p.K + (size_t)cslot * p.kv_bstride + (size_t)kvh * 128 + 8 * j;
  const bf16_t* Vb = KV8 ? nullptr : p.V + (size_t)cslot * p.kv_bstride + (size_t)kvh * 128 + 8 * j;
  const uint8_t* Kb8 = KV8 ? p.K8 + (size_t)cslot * p.kv_bstride + (size_t)kvh * 128 + 8 * j : nullptr;
  const uint8_t* Vb8 = KV8 ? p.V8 + (size_t)cslot * p.kv_bstride + (size_t)kvh * 128 + 8 * j : nullptr;
  const float* Ksb = KV8 ? p.k_scale + (size_t)cslot * p.s_bstride + kvh : nullptr;
  const float* Vsb = KV8 ? p.v_scale + (size_t)cslot * p.s_bstride + kvh : nullptr;
  u32x4_t q[T][G];
#pragma unroll
  for (int r = 0; r < T; ++r) {
    const size_t rr = qrow + (r < tc ? r : 0);      // (a row past the chunk repeats its first row: loaded, never used)
#pragma unroll
    for (int g = 0; g < G; ++g) q[r][g] = *(const u32x4_t*)(p.Q + rr * p.ldq + (size_t)(qg * G + g) * 128 + 8 * j);
  }
  float m[T][G], l[T][G], o[T][G][8];
#pragma unroll
  for (int r = 0; r < T; ++r)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      m[r][g] = -INFINITY; l[r][g] = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[r][g][i] = 0.f;
    }
  const float sc = p.scale * 1.4426950408889634f;
  auto one_key_f = [&](const u32x4_t& kk, const float (&vf)[8], const int key) {
#pragma unroll
    for (int r = 0; r < T; ++r) {
      if (r < tc && key < len_first + r) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          // the single-row kernel's expressions with the contractions the compiler makes there WRITTEN OUT (it fuses s - mn into fma(dot, sc, -mn),
          // l corr + pe and pe v + (o corr)): under a predicate it would otherwise be free to fuse them another way, and the bits would differ
          const float dot = row16_sum(dot8(kk, q[r][g], 0.f));
          const float mn = fmaxf(m[r][g], dot * sc);
          const float corr = __builtin_amdgcn_exp2f(m[r][g] - mn), pe = __builtin_amdgcn_exp2f(__builtin_fmaf(dot, sc, -mn));
          m[r][g] = mn;
          l[r][g] = __builtin_fmaf(l[r][g], corr, pe);
#pragma unroll
          for (int i = 0; i < 8; ++i) o[r][g][i] = __builtin_fmaf(pe, vf[i], o[r][g][i] * corr);
        }
      }
    }
  };
  auto fetch = [&](int key) -> KeyRaw {
    if constexpr (KV8) {
      return KeyRaw8{*(const u32x2_t*)(Kb8 + (size_t)key * p.ldkv), *(const u32x2_t*)(Vb8 + (size_t)key * p.ldkv), Ksb[(size_t)key * p.lds], Vsb[(size_t)key * p.lds]};
    } else {
      return KeyRaw16{*(const u32x4_t*)(Kb + (size_t)key * p.ldkv), *(const u32x4_t*)(Vb + (size_t)key * p.ldkv)};
    }
  };
  auto use = [&](const KeyRaw& r, const int key) {
    float vf[8];
    if constexpr (KV8) {
      e4m3p2_to_f32(r.v, r.vs, vf);
      one_key_f(e4m3p2_to_bf16(r.k, r.ks), vf, key);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) { vf[2 * i] = bf_lo(r.v[i]); vf[2 * i + 1] = bf_hi(r.v[i]); }
      one_key_f(r.k, vf, key);
    }
  };
  constexpr int UN = S >= 6 ? 2 : 4;      // as above: two keys per buffer keep 6 .. 8 states inside 256 registers
  int key = slot;
  if (key + 16 * (UN - 1) < len_last) {
    KeyRaw r[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) r[u] = fetch(key + 16 * u);
    for (;;) {
      const int nkey = key + 16 * UN;
      const bool more = nkey + 16 * (UN - 1) < len_last;
      KeyRaw rn[UN];
      if (more) {
#pragma unroll
        for (int u = 0; u < UN; ++u) rn[u] = fetch(nkey + 16 * u);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) use(r[u], key + 16 * u);
      key = nkey;
      if (!more) break;
#pragma unroll
      for (int u = 0; u < UN; ++u) r[u] = rn[u];
    }
  }
  for (; key < len_last; key += 16) use(fetch(key), key);
#pragma unroll
  for (int r = 0; r < T; ++r)
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        const float mo = __shfl_xor(m[r][g], off, 64), lo = __shfl_xor(l[r][g], off, 64);
        const float mn = fmaxf(m[r][g], mo);
        const float ca = m[r][g] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[r][g] - mn);
        const float cb = mo == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mo - mn);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[r][g][i] = __builtin_fmaf(o[r][g][i], ca, __shfl_xor(o[r][g][i], off, 64) * cb);
        l[r][g] = __builtin_fmaf(l[r][g], ca, lo * cb);
        m[r][g] = mn;
      }
      if (lane < 16) {
        if (lane == 0) { sm_m[wid][r * G + g] = m[r][g]; sm_l[wid][r * G + g] = l[r][g]; }
#pragma unroll
        for (int i = 0; i < 8; ++i) sm_o[wid][r * G + g][8 * j + i] = o[r][g][i];
      }
    }
  __syncthreads();
  for (int e = tid; e < tc * G * 128; e += 256) {
    const int st = e >> 7, d = e & 127;      // state = row * G + head
    const int r = st / G, g = st - r * G;
    float mn = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mn = fmaxf(mn, sm_m[w][st]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float c = sm_m[w][st] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sm_m[w][st] - mn);
      num = __builtin_fmaf(sm_o[w][st][d], c, num);
      den = __builtin_fmaf(sm_l[w][st], c, den);
    }
    p.O[(qrow + r) * p.ldo + (size_t)(qg * G + g) * 128 + d] = f2bf(den > 0.f ? num / den : 0.f);
  }
}

}  // namespace

static std::atomic<int> g_decode_group{0};
extern "C" int td_attention_decode_set_group(int g) { return g_decode_group.exchange(g); }

int td_attn_decode_launch(const TdAttnParams& p, hipStream_t stream) {
  TD_CHECK_ARG(p.Sq == 1 && p.head_dim == 128 && p.Hq % p.Hkv == 0, "td_attn_decode: needs Sq = 1, head_dim 128");
  TdAttnParams q = p;
  q.q_per_kv = p.Hq / p.Hkv;
  if (p.dec_kv_new) TD_CHECK_ARG(p.kv_lens && p.dec_cos && p.dec_sin && p.dec_row_off && ((uintptr_t)p.dec_kv_new | (uintptr_t)p.dec_cos | (uintptr_t)p.dec_sin) % 16 == 0,
                                 "td_attn_decode: the fused rotary / cache-write form needs kv_lens, both table rows and the cache row offsets");
  const bool kv8 = p.K8 != nullptr;
  if (kv8) {
    TD_CHECK_ARG(p.V8 && p.k_scale && p.v_scale && p.Q && p.O, "td_attn_decode: the e4m3 cache form needs both byte planes and both scale planes");
    TD_CHECK_ARG(p.ldkv % 8 == 0 && p.kv_bstride % 8 == 0 && ((uintptr_t)p.K8 | (uintptr_t)p.V8) % 8 == 0 && ((uintptr_t)p.k_scale | (uintptr_t)p.v_scale) % 4 == 0 &&
                 ((uintptr_t)p.Q | (uintptr_t)p.O) % 16 == 0 && p.q_bstride % 8 == 0 && p.lds > 0,
                 "td_attn_decode: e4m3 cache lines must be 8-byte aligned (ldkv %% 8 == 0 bytes), scales 4-byte, q and o 16-byte");
  } else
  TD_CHECK_ARG(p.ldkv % 8 == 0 && ((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V | (uintptr_t)p.O) % 16 == 0 && p.q_bstride % 8 == 0 && p.kv_bstride % 8 == 0,
               "td_attn_decode: operands must be 16-byte aligned");
  // G q heads of one kv head per workgroup read its K/V once instead of G times (from L2); taken when the grid still gives
  // every CU a workgroup -- many sequences -- and left at one head per workgroup for small batches
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    static std::atomic<int> cached[64] = {};
    int n = cached[dev & 63].load(std::memory_order_relaxed);
    if (n == 0 && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) cached[dev & 63].store(n, std::memory_order_relaxed);
    if (n > 0) cus = n;
  }
  const int forced = g_decode_group.load(std::memory_order_relaxed);      // td_attention_decode_set_group: tests and A/B
  int G = 1;
  for (int g : {7, 6, 4, 3, 2})
    if (q.q_per_kv % g == 0 && (forced ? g == forced : (long long)(p.Hq / g) * p.batch >= cus)) { G = g; break; }
  const dim3 grid(p.Hq / G, p.batch);
#define TD_DEC_LAUNCH(g)                                                                                        \
  do {                                                                                                          \
    if (kv8) hipLaunchKernelGGL((td_attn_decode_kernel<g, true>), grid, dim3(256), 0, stream, q);               \
    else hipLaunchKernelGGL((td_attn_decode_kernel<g, false>), grid, dim3(256), 0, stream, q);                  \
  } while (0)
  switch (G) {
    case 7: TD_DEC_LAUNCH(7); break;
    case 6: TD_DEC_LAUNCH(6); break;
    case 4: TD_DEC_LAUNCH(4); break;
    case 3: TD_DEC_LAUNCH(3); break;
    case 2: TD_DEC_LAUNCH(2); break;
    default: TD_DEC_LAUNCH(1);
  }
#undef TD_DEC_LAUNCH
  TD_CHECK_LAUNCH();
  return 0;
}

static std::atomic<int> g_verify_form{0};
extern "C" int td_attention_verify_set_form(int form) { return g_verify_form.exchange(form); }

int td_attn_verify_launch(const TdAttnParams& p, int t_max, hipStream_t stream) {
  int dev = 0, cus = 256;
  // every refusal before the first HIP call
  const bool kv8 = p.K8 != nullptr;
  TD_CHECK_ARG(p.Q && p.O, "td_attention_verify: null q (%p) or o (%p)", (const void*)p.Q, (const void*)p.O);
  TD_CHECK_ARG(p.vr_row0 && p.vr_rows && p.vr_len0 && p.vr_slot, "td_attention_verify: null per-sequence array (row0 %p, rows %p, len0 %p, slot %p)",
               (const void*)p.vr_row0, (const void*)p.vr_rows, (const void*)p.vr_len0, (const void*)p.vr_slot);
  TD_CHECK_ARG((p.K != nullptr || p.V != nullptr) != (p.K8 != nullptr || p.V8 != nullptr || p.k_scale != nullptr || p.v_scale != nullptr),
               "td_attention_verify: exactly one cache form is needed: bf16 (k %p, v %p) or e4m3 (k8 %p, v8 %p, k_scale %p, v_scale %p)", (const void*)p.K,
               (const void*)p.V, (const void*)p.K8, (const void*)p.V8, (const void*)p.k_scale, (const void*)p.v_scale);
  if (kv8) TD_CHECK_ARG(p.K8 && p.V8 && p.k_scale && p.v_scale, "td_attention_verify: the e4m3 form needs both byte planes and both scale planes (k8 %p, v8 %p, k_scale %p, v_scale %p)",
                        (const void*)p.K8, (const void*)p.V8, (const void*)p.k_scale, (const void*)p.v_scale);
  else TD_CHECK_ARG(p.K && p.V, "td_attention_verify: the bf16 form needs k (%p) and v (%p)", (const void*)p.K, (const void*)p.V);
  TD_CHECK_ARG(p.batch >= 1 && p.batch <= 256, "td_attention_verify: n_seq=%d outside 1..256", p.batch);
  TD_CHECK_ARG(p.Hq > 0 && p.Hkv > 0 && p.Hq % p.Hkv == 0, "td_attention_verify: Hq=%d is not a positive multiple of Hkv=%d", p.Hq, p.Hkv);
  TD_CHECK_ARG(t_max >= 1 && t_max <= TD_MAX_VERIFY_ROWS, "td_attention_verify: t_max=%d outside 1..%d", t_max, TD_MAX_VERIFY_ROWS);
  TD_CHECK_ARG(p.ldq % 8 == 0 && p.ldo % 8 == 0 && p.ldq >= p.Hq * 128 && p.ldo >= p.Hq * 128 && ((uintptr_t)p.Q | (uintptr_t)p.O) % 16 == 0,
               "td_attention_verify: ldq=%d, ldo=%d must be multiples of 8 and at least Hq x 128 = %d, q and o 16-byte aligned", p.ldq, p.ldo, p.Hq * 128);
  TD_CHECK_ARG(p.ldkv % 8 == 0 && p.kv_bstride % 8 == 0 && p.ldkv >= p.Hkv * 128 && p.kv_bstride >= 0,
               "td_attention_verify: ldkv=%d, kv_bstride=%lld must be multiples of 8, ldkv at least Hkv x 128 = %d", p.ldkv, p.kv_bstride, p.Hkv * 128);
  if (kv8) TD_CHECK_ARG(((uintptr_t)p.K8 | (uintptr_t)p.V8) % 8 == 0 && ((uintptr_t)p.k_scale | (uintptr_t)p.v_scale) % 4 == 0 && p.lds >= p.Hkv && p.s_bstride >= 0,
                        "td_attention_verify: e4m3 cache lines must be 8-byte aligned, scales 4-byte, lds=%d at least Hkv=%d", p.lds, p.Hkv);
  else TD_CHECK_ARG(((uintptr_t)p.K | (uintptr_t)p.V) % 16 == 0, "td_attention_verify: k (%p) and v (%p) must be 16-byte aligned", (const void*)p.K, (const void*)p.V);
  TD_CHECK_ARG(((uintptr_t)p.vr_row0 | (uintptr_t)p.vr_rows | (uintptr_t)p.vr_len0 | (uintptr_t)p.vr_slot) % 4 == 0, "td_attention_verify: the per-sequence arrays must be 4-byte aligned");
  const int qpk = p.Hq / p.Hkv;
  if (hipGetDevice(&dev) == hipSuccess) {
    const int n = td_attn_device_cus(dev);
    if (n > 0) cus = n;
  }
  const int forced = g_decode_group.load(std::memory_order_relaxed);      // td_attention_decode_set_group: tests and A/B
  int form = g_verify_form.load(std::memory_order_relaxed);
  // Automatic, as measured (tools/bench_spec_decode.py, profiles/spec_decode_bench.json).  The kernel is bound by its arithmetic, not by the K/V bytes --
  // in the row form the repeated reads come from L2 -- so spreading the rows over workgroups wins almost everywhere: the multi-row kernel costs
  // x1.0 - 3.3 of the row form at 8 rows per sequence, at one sequence below 4096 keys, and wherever the (head, sequence) grid alone fills the chip.
  // It is taken where it measured faster, always with 2 .. 4 rows per sequence and Hq x sequences < CUs; p.Skv = the longest visible length (0: the
  // caller does not know it, which counts as short):
  //   e4m3 cache, 2 rows:      from 4096 keys on (x0.64 - 0.79), and from 1024 keys on with 8 or more sequences (x0.66 - 0.75 at 2048)
  //   e4m3 cache, 3 - 4 rows:  8 or more sequences (x0.54 - 0.84 at 28 q heads, level at 12)
  //   bf16 cache:              from 4096 keys on while the grid fills at least half the chip (x0.82 - 0.86 at 28 heads x 8 sequences)
  if (form != 1 && form != 2) {
    const long long wg = (long long)p.Hq * p.batch;
    bool multi = false;
    if (wg < cus && t_max >= 2 && t_max <= 4) {
      if (kv8) multi = t_max == 2 ? (p.Skv >= 4096 || (p.Skv >= 1024 && p.batch >= 8)) : p.batch >= 8;
      else multi = p.Skv >= 4096 && 2 * wg >= cus;
    }
    form = multi ? 2 : 1;
  }
  if (form == 1) {
    TdAttnParams q = p;
    q.q_per_kv = qpk; q.vr_tmax = t_max; q.q_bstride = p.ldq; q.o_bstride = p.ldo;
    int G = 1;
    for (int g : {7, 6, 4, 3, 2})
      if (qpk % g == 0 && (forced ? g == forced : (long long)(p.Hq / g) * p.batch * t_max >= cus)) { G = g; break; }
    const dim3 grid(p.Hq / G, p.batch * t_max);
#define TD_VR_LAUNCH(g)                                                                                              \
  do {                                                                                                               \
    if (kv8) hipLaunchKernelGGL((td_attn_decode_kernel<g, true, true>), grid, dim3(256), 0, stream, q);              \
    else hipLaunchKernelGGL((td_attn_decode_kernel<g, false, true>), grid, dim3(256), 0, stream, q);                 \
  } while (0)
    switch (G) {
      case 7: TD_VR_LAUNCH(7); break;
      case 6: TD_VR_LAUNCH(6); break;
      case 4: TD_VR_LAUNCH(4); break;
      case 3: TD_VR_LAUNCH(3); break;
      case 2: TD_VR_LAUNCH(2); break;
      default: TD_VR_LAUNCH(1);
    }
#undef TD_VR_LAUNCH
    TD_CHECK_LAUNCH();
    return 0;
  }
  // the multi-row kernel: the largest G that still gives every CU a workgroup (the single-row rule), under G x T <= 8 with T the smallest of 2, 4, 8
  // that holds t_max rows; a G that leaves no room for T rows (a forced 6 or 7, or 3 / 4 with more than two rows) walks the rows in chunks of T
  const int T_want = t_max <= 1 ? 1 : t_max <= 2 ? 2 : t_max <= 4 ? 4 : 8;
  int G = 1;
  for (int g : {7, 6, 4, 3, 2})
    if (qpk % g == 0 && (forced ? g == forced : (g * T_want <= 8 && (long long)(p.Hq / g) * p.batch >= cus))) { G = g; break; }
  const int T_room = G >= 5 ? 1 : G >= 3 ? 2 : G == 2 ? 4 : 8;
  const int T = T_want < T_room ? (T_want < 2 && G < 5 ? 2 : T_want) : T_room;
  TdAttnVerifyParams v;
  v.Q = p.Q; v.O = p.O; v.K = p.K; v.V = p.V; v.K8 = p.K8; v.V8 = p.V8; v.k_scale = p.k_scale; v.v_scale = p.v_scale;
  v.ldq = p.ldq; v.ldkv = p.ldkv; v.ldo = p.ldo; v.lds = p.lds; v.kv_bstride = p.kv_bstride; v.s_bstride = p.s_bstride;
  v.row0 = p.vr_row0; v.rows = p.vr_rows; v.len0 = p.vr_len0; v.slot = p.vr_slot; v.q_per_kv = qpk; v.t_max = t_max; v.scale = p.scale;
  const dim3 grid(p.Hq / G, p.batch, (t_max + T - 1) / T);
#define TD_VF_LAUNCH(g, t)                                                                                           \
  do {                                                                                                               \
    if (kv8) hipLaunchKernelGGL((td_attn_verify_kernel<g, t, true>), grid, dim3(256), 0, stream, v);                 \
    else hipLaunchKernelGGL((td_attn_verify_kernel<g, t, false>), grid, dim3(256), 0, stream, v);                    \
  } while (0)
  switch (G * 16 + T) {
    case 7 * 16 + 1: TD_VF_LAUNCH(7, 1); break;
    case 6 * 16 + 1: TD_VF_LAUNCH(6, 1); break;
    case 4 * 16 + 2: TD_VF_LAUNCH(4, 2); break;
    case 3 * 16 + 2: TD_VF_LAUNCH(3, 2); break;
    case 2 * 16 + 2: TD_VF_LAUNCH(2, 2); break;
    case 2 * 16 + 4: TD_VF_LAUNCH(2, 4); break;
    case 1 * 16 + 2: TD_VF_LAUNCH(1, 2); break;
    case 1 * 16 + 4: TD_VF_LAUNCH(1, 4); break;
    case 1 * 16 + 8: TD_VF_LAUNCH(1, 8); break;
    default: TD_CHECK_ARG(false, "td_attention_verify: no kernel for G=%d, T=%d", G, T);
  }
#undef TD_VF_LAUNCH
  TD_CHECK_LAUNCH();
  return 0;
}

// ---- the rows of an e4m3 KV cache: bf16 k | v rows -> bytes + scales, and back ------------------------------------------------------------------
namespace {

// 16 lanes per head vector (lane j: elements 8j .. 8j+7), 16 vectors per workgroup.  A vector past the end is clamped to the last one and stores
// nothing, so every DPP row is fully active.  kv_hat may alias kv: a row of lanes reads its vector before it writes it, and nobody else touches it.
__global__ __launch_bounds__(256) void td_kv_quant_rows_kernel(const bf16_t* kv, long long ld, uint8_t* q, long long ldq, float* scale, long long lds,
                                                               bf16_t* kv_hat, long long total, int heads, const int* dst_rows) {
  const long long unit = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = unit < total;
  const long long u = live ? unit : total - 1;
  const long long r = u / heads;
  const int h = (int)(u - r * heads), j = threadIdx.x & 15;
  u32x4_t x = *(const u32x4_t*)(kv + (size_t)r * ld + (size_t)h * 128 + 8 * j);
  float s;
  const u32x2_t b = kv8_round_row(x, s);
  if (!live) return;
  const size_t dr = dst_rows ? (size_t)dst_rows[r] : (size_t)r;
  *(u32x2_t*)(q + dr * ldq + (size_t)h * 128 + 8 * j) = b;
  if (j == 0) scale[dr * lds + h] = s;
  if (kv_hat) *(u32x4_t*)(kv_hat + (size_t)r * ld + (size_t)h * 128 + 8 * j) = x;
}

__global__ __launch_bounds__(256) void td_kv_dequant_rows_kernel(const uint8_t* q, long long ldq, const float* scale, long long lds, bf16_t* out, long long ld,
                                                                 long long total, int heads) {
  const long long unit = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (unit >= total) return;
  const long long r = unit / heads;
  const int h = (int)(unit - r * heads), j = threadIdx.x & 15;
  const u32x2_t b = *(const u32x2_t*)(q + (size_t)r * ldq + (size_t)h * 128 + 8 * j);
  *(u32x4_t*)(out + (size_t)r * ld + (size_t)h * 128 + 8 * j) = e4m3p2_to_bf16(b, scale[(size_t)r * lds + h]);
}

// ... row-mapped: out row r = cache row src_rows[r] (device ints): the rows of several sequences gathered into one packed staging buffer in one launch
__global__ __launch_bounds__(256) void td_kv_dequant_rows_from_kernel(const uint8_t* q, long long ldq, const float* scale, long long lds, bf16_t* out, long long ld,
                                                                      long long total, int heads, const int* src_rows) {
  const long long unit = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (unit >= total) return;
  const long long r = unit / heads;
  const int h = (int)(unit - r * heads), j = threadIdx.x & 15;
  const size_t sr = (size_t)max(src_rows[r], 0);
  const u32x2_t b = *(const u32x2_t*)(q + sr * ldq + (size_t)h * 128 + 8 * j);
  *(u32x4_t*)(out + (size_t)r * ld + (size_t)h * 128 + 8 * j) = e4m3p2_to_bf16(b, scale[sr * lds + h]);
}

}  // namespace

int td_kv_quant_rows_launch(const bf16_t* kv, long long ld, uint8_t* q, long long ldq, float* scale, long long lds, bf16_t* kv_hat, int rows, int heads,
                            const int* dst_rows, hipStream_t stream) {
  TD_CHECK_ARG(kv && q && scale, "td_kv_quant_rows_e4m3: kv, q and scale are required");
  TD_CHECK_ARG(heads > 0 && rows > 0, "td_kv_quant_rows_e4m3: rows=%d, heads=%d must be positive", rows, heads);
  TD_CHECK_ARG(ld >= (long long)heads * 128 && ld % 8 == 0 && ldq >= (long long)heads * 128 && ldq % 8 == 0 && lds >= heads,
               "td_kv_quant_rows_e4m3: ld=%lld, ldq=%lld must be multiples of 8 and at least heads x 128 = %lld, lds=%lld at least heads", ld, ldq, (long long)heads * 128, lds);
  TD_CHECK_ARG((uintptr_t)kv % 16 == 0 && (uintptr_t)kv_hat % 16 == 0 && (uintptr_t)q % 8 == 0 && (uintptr_t)scale % 4 == 0 && (uintptr_t)dst_rows % 4 == 0,
               "td_kv_quant_rows_e4m3: misaligned rows: kv and kv_hat must be 16-byte aligned, q 8-byte, scale and dst_rows 4-byte");
  const long long total = (long long)rows * heads;
  hipLaunchKernelGGL(td_kv_quant_rows_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, stream, kv, ld, q, ldq, scale, lds, kv_hat, total, heads, dst_rows);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_kv_dequant_rows_launch(const uint8_t* q, long long ldq, const float* scale, long long lds, bf16_t* out, long long ld, int rows, int heads, hipStream_t stream) {
  TD_CHECK_ARG(q && scale && out, "td_kv_dequant_rows_e4m3: q, scale and out are required");
  TD_CHECK_ARG(heads > 0 && rows > 0, "td_kv_dequant_rows_e4m3: rows=%d, heads=%d must be positive", rows, heads);
  TD_CHECK_ARG(ld >= (long long)heads * 128 && ld % 8 == 0 && ldq >= (long long)heads * 128 && ldq % 8 == 0 && lds >= heads,
               "td_kv_dequant_rows_e4m3: ld=%lld, ldq=%lld must be multiples of 8 and at least heads x 128 = %lld, lds=%lld at least heads", ld, ldq, (long long)heads * 128, lds);
  TD_CHECK_ARG((uintptr_t)out % 16 == 0 && (uintptr_t)q % 8 == 0 && (uintptr_t)scale % 4 == 0,
               "td_kv_dequant_rows_e4m3: misaligned rows: out must be 16-byte aligned, q 8-byte, scale 4-byte");
  const long long total = (long long)rows * heads;
  hipLaunchKernelGGL(td_kv_dequant_rows_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, stream, q, ldq, scale, lds, out, ld, total, heads);
  TD_CHECK_LAUNCH();
  return 0;
}

// out row r = the dequantised cache row src_rows[r] (device ints, the caller vouches that they name rows of q / scale; a negative one counts as 0)
int td_kv_dequant_rows_from_launch(const uint8_t* q, long long ldq, const float* scale, long long lds, bf16_t* out, long long ld, int rows, int heads,
                                   const int* src_rows, hipStream_t stream) {
  TD_CHECK_ARG(q && scale && out && src_rows, "td_kv_dequant_rows_from: q, scale, out and src_rows are required");
  TD_CHECK_ARG(heads > 0 && rows > 0, "td_kv_dequant_rows_from: rows=%d, heads=%d must be positive", rows, heads);
  TD_CHECK_ARG(ld >= (long long)heads * 128 && ld % 8 == 0 && ldq >= (long long)heads * 128 && ldq % 8 == 0 && lds >= heads,
               "td_kv_dequant_rows_from: ld=%lld, ldq=%lld must be multiples of 8 and at least heads x 128 = %lld, lds=%lld at least heads", ld, ldq, (long long)heads * 128, lds);
  TD_CHECK_ARG((uintptr_t)out % 16 == 0 && (uintptr_t)q % 8 == 0 && (uintptr_t)scale % 4 == 0 && (uintptr_t)src_rows % 4 == 0,
               "td_kv_dequant_rows_from: misaligned rows: out must be 16-byte aligned, q 8-byte, scale and src_rows 4-byte");
  const long long total = (long long)rows * heads;
  hipLaunchKernelGGL(td_kv_dequant_rows_from_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, stream, q, ldq, scale, lds, out, ld, total, heads, src_rows);
  TD_CHECK_LAUNCH();
  return 0;
}
