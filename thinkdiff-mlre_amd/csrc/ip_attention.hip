// FLUX IP-Adapter cross-attention (td_ip_attention_bf16): the image rows' query attends to a handful of image-prompt tokens and the scaled
// result is written -- or added -- to a [rows, D] buffer ([ext] diffusers FluxIPAdapterJointAttnProcessor2_0, restated; parity unpinned).
//
//   o[m, h*128 + d] = (accumulate ? o[m, h*128 + d] : 0) (+) bf16(out_scale * float(bf16(sum_j P[m, h, j] v[j, h*128 + d])))
//   P = softmax_j(qn[m, h, :] . k[j, h, :] * 128^-0.5), j < n_keys;   qn = norm_w ? bf16(bf16(q * rstd) * w) : q
//
// One launch, grid (query-row tile, head), 4 waves of 16 query rows each per pass.  What the design follows from:
//  * the QK-RMSNorm of q is fused: the engine's q is normalised AND rotated in place by td_qk_norm_rope, and the IP query is the normalised,
//    un-rotated one -- nobody holds it.  The kernel reads the raw projection and applies qk_norm8 (csrc/qk_rope_math.h) with that kernel's
//    summation tree (16 partial sums of 8 elements, xor-butterfly 8, 4, 2, 1), so qn has the bits td_qk_norm_rope rounds before rotating;
//  * to_k_ip's output is NOT normalised, so no score bound holds: the softmax uses the TRUE row maximum.  All keys of a head (<= 256) are
//    scored before the first exponential, so the maximum is exact and there is no rescaling chain;
//  * K and V of the head are staged in LDS once per workgroup, rows n_keys .. keys_pad ZERO-FILLED there (never read from the caller), and the
//    padded scores are set to -inf before the maximum: padding is masked, not read as data;
//  * both products run on v_mfma_f32_16x16x32_bf16, swapped: S^T[key][q] = K . Q^T leaves a query row on ONE lane column (l & 15), its keys in
//    the 4 accumulator registers x the 4 lane groups, and those registers -- rounded to bf16 -- ARE the B operand of O^T[d][q] = V^T . P^T.
//    The contraction order of that product is free as long as both operands agree: k-slot 8g + j of pair u is key 32u + 4g + j (j < 4) or
//    32u + 16 + 4g + j - 4, which is what lane group g already holds of tiles 2u and 2u + 1;
//  * V^T fragments come from the row-major LDS image by ds_read_b64_tr_b16; the 16 rows of the A operand are assigned to head columns
//    d = 32 (r >> 2) + 4 dt + (r & 3), so a lane ends up with 32 CONTIGUOUS columns of its query row (four 16-byte stores, 256 B per row over the
//    4 lane groups).  q is read the same way (lane group g: columns 32g .. 32g + 31; the k-steps of QK^T are permuted to match);
//  * LDS rows: K 272 B (ds_read_b128 of 16 keys x one 16-byte chunk: 4 banks per key apart), V 264 B (the transposed read of a 32-lane half
//    takes 8 key rows x 4 column blocks: 2 banks per row + 16 per block, conflict-free by the 64-bank rule).
// HBM-bound by construction (FLUX.1-dev at 1024^2: 25 MB of q read, 25 MB written per block); the MFMA fill at 4 keys does not matter.
#include <atomic>
#include <cmath>

#include "qk_rope_math.h"
#include "td_kernels.h"
#include "../../include/thinkdiff_hip.h"

namespace {

constexpr int K_STRIDE = 272;      // bytes per staged key row
constexpr int V_STRIDE = 264;      // bytes per staged value row (8-byte aligned: the transposed read's requirement)

struct IpParams {
  const bf16_t *q, *k, *v, *w;
  bf16_t* o;
  int rows, H, n_keys, ldq, ldkv, ldo;
  float out_scale, eps;
  int accumulate, passes;      // passes: 64-row passes per workgroup
};

__device__ __forceinline__ void ip_unpack8(const u32x4_t r, float (&x)[8]) {
  x[0] = bf_lo(r.x); x[1] = bf_hi(r.x); x[2] = bf_lo(r.y); x[3] = bf_hi(r.y);
  x[4] = bf_lo(r.z); x[5] = bf_hi(r.z); x[6] = bf_lo(r.w); x[7] = bf_hi(r.w);
}
// two transposed reads 16 value rows apart = one V^T fragment; the wait sits inside (the compiler does not count an asm's LDS reads)
__device__ __forceinline__ bf16x8_t ip_read_vt(const unsigned addr) {
  bf16x4_t lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%3\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(lo), "=&v"(hi) : "v"(addr), "n"(16 * V_STRIDE));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// NP: pairs of 16-key tiles -- keys_pad = 32 NP keys are scored, n_keys of them real
template <int NP>
__global__ __launch_bounds__(256) void td_ip_attention_kernel(const IpParams p) {
  extern __shared__ __attribute__((aligned(16))) char ip_lds[];
  constexpr int KP = 32 * NP;
  char* const ks = ip_lds;
  char* const vs = ip_lds + KP * K_STRIDE;
  const int head = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = lane & 15, g = lane >> 4;

  // ---- stage K and V of this head: 16-byte chunks, rows >= n_keys are zeros -----------------------------------------------------------
  {
    const bf16_t* kg = p.k + (size_t)head * 128;
    const bf16_t* vg = p.v + (size_t)head * 128;
    for (int c = tid; c < KP * 16; c += 256) {
      const int row = c >> 4, ch = c & 15;
      u32x4_t kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
      if (row < p.n_keys) {
        kv = *(const u32x4_t*)(kg + (size_t)row * p.ldkv + ch * 8);
        vv = *(const u32x4_t*)(vg + (size_t)row * p.ldkv + ch * 8);
      }
      *(u32x4_t*)(ks + row * K_STRIDE + ch * 16) = kv;
      u32x2_t* vd = (u32x2_t*)(vs + row * V_STRIDE + ch * 16);
      vd[0] = u32x2_t{vv.x, vv.y};
      vd[1] = u32x2_t{vv.z, vv.w};
    }
  }
  __syncthreads();

  float wv[4][8];
  if (p.w) {
#pragma unroll
    for (int s = 0; s < 4; ++s) ip_unpack8(*(const u32x4_t*)(p.w + 32 * g + 8 * s), wv[s]);
  }
  const unsigned ks_base = (unsigned)(uintptr_t)(TD_LDS char*)ks + qi * K_STRIDE + 64 * g;
  // transposed read: lane 4q' + pb of a 16-lane group supplies row q' of the 4-key block, columns 32 pb + 4 dt .. + 3
  const unsigned vs_base = (unsigned)(uintptr_t)(TD_LDS char*)vs + (4 * g + (qi >> 2)) * V_STRIDE + 64 * (qi & 3);
  const float c2 = 0.08838834764831845f * 1.4426950408889634f;      // 128^-0.5 log2(e)
  const int row_base = blockIdx.x * 64 * p.passes;

  for (int pass = 0; pass < p.passes; ++pass) {
    const int r0 = row_base + (pass * 4 + wave) * 16;      // wave-uniform: the whole wave leaves together (the transposed reads need EXEC all ones)
    if (r0 >= p.rows) break;
    const int row = r0 + qi;
    const int row_c = row < p.rows ? row : p.rows - 1;     // rows past the end compute a copy of the last row and store nothing
    // ---- q: columns 32g .. 32g + 31 of the lane's row; k-step s of QK^T contracts columns 32g + 8s + j ---------------------------------
    const bf16_t* qp = p.q + (size_t)row_c * p.ldq + (size_t)head * 128 + 32 * g;
    u32x4_t raw[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) raw[s] = *(const u32x4_t*)(qp + 8 * s);
    bf16x8_t qf[4];
    if (p.w) {
      float x[4][8], part[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) { ip_unpack8(raw[s], x[s]); part[s] = qk_sumsq8(x[s]); }
      // td_qk_norm_rope's tree over the 16 chunks c = 4g + s: xor 8 (lane group g ^ 2), xor 4 (g ^ 1), xor 2 and xor 1 (in the lane)
#pragma unroll
      for (int s = 0; s < 4; ++s) part[s] += __shfl_xor(part[s], 32, 64);
#pragma unroll
      for (int s = 0; s < 4; ++s) part[s] += __shfl_xor(part[s], 16, 64);
      const float rstd = qk_rstd((part[0] + part[2]) + (part[1] + part[3]), p.eps);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        qk_norm8(x[s], rstd, wv[s]);
        u32x4_t pk;      // (already bf16 values: their upper halves are the bits)
        pk.x = (as_u32(x[s][0]) >> 16) | (as_u32(x[s][1]) & 0xffff0000u);
        pk.y = (as_u32(x[s][2]) >> 16) | (as_u32(x[s][3]) & 0xffff0000u);
        pk.z = (as_u32(x[s][4]) >> 16) | (as_u32(x[s][5]) & 0xffff0000u);
        pk.w = (as_u32(x[s][6]) >> 16) | (as_u32(x[s][7]) & 0xffff0000u);
        qf[s] = __builtin_bit_cast(bf16x8_t, pk);
      }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) qf[s] = __builtin_bit_cast(bf16x8_t, raw[s]);
    }

    // ---- S^T = K . Q^T: tile t, register i of lane group g = key 16t + 4g + i against query row qi --------------------------------------
    f32x4_t sc[2 * NP];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2 * NP; ++t) {
      f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8_t kf = *(const TD_LDS bf16x8_t*)(uintptr_t)(ks_base + t * 16 * K_STRIDE + 16 * s);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], a, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = (16 * t + 4 * g + i < p.n_keys) ? a[i] : -INFINITY;      // the padding is masked
        a[i] = v;
        mx = fmaxf(mx, v);
      }
      sc[t] = a;
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // the row's true maximum (n_keys >= 1: finite)
    // ---- P = exp2((s - max) c), rounded to bf16 for the second product; the row sum is over the rounded values ---------------------------
    bf16x8_t pf[NP];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      float e[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        e[i] = rbf(__builtin_amdgcn_exp2f((sc[2 * u][i] - mx) * c2));
        e[4 + i] = rbf(__builtin_amdgcn_exp2f((sc[2 * u + 1][i] - mx) * c2));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) sum += e[i];
      u32x4_t pk;
      pk.x = (as_u32(e[0]) >> 16) | (as_u32(e[1]) & 0xffff0000u);
      pk.y = (as_u32(e[2]) >> 16) | (as_u32(e[3]) & 0xffff0000u);
      pk.z = (as_u32(e[4]) >> 16) | (as_u32(e[5]) & 0xffff0000u);
      pk.w = (as_u32(e[6]) >> 16) | (as_u32(e[7]) & 0xffff0000u);
      pf[u] = __builtin_bit_cast(bf16x8_t, pk);
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;

    // ---- O^T = V^T . P^T: tile dt, register i of lane group g = head column 32g + 4dt + i of query row qi ---------------------------------
    f32x4_t acc[8];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        const bf16x8_t vf = ip_read_vt(vs_base + u * 32 * V_STRIDE + 8 * dt);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[u], a, 0, 0, 0);
      }
      acc[dt] = a;
    }

    // ---- epilogue: bf16(sum P v), x out_scale, rounded; one bf16 add onto o when accumulating ------------------------------------------------
    if (row < p.rows) {
      bf16_t* op = p.o + (size_t)row * p.ldo + (size_t)head * 128 + 32 * g;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float y[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = rbf(p.out_scale * rbf(acc[2 * c + (i >> 2)][i & 3] * inv));
        if (p.accumulate) {
          float old[8];
          ip_unpack8(*(const u32x4_t*)(op + 8 * c), old);
#pragma unroll
          for (int i = 0; i < 8; ++i) y[i] = old[i] + y[i];
        }
        u32x4_t pk;
        pk.x = pack_bf2(y[0], y[1]); pk.y = pack_bf2(y[2], y[3]); pk.z = pack_bf2(y[4], y[5]); pk.w = pack_bf2(y[6], y[7]);
        *(u32x4_t*)(op + 8 * c) = pk;
      }
    }
  }
}

template <int NP>
int launch_np(const IpParams& p, hipStream_t s) {
  static std::atomic<unsigned long long> done{0};
  constexpr int lds = 32 * NP * (K_STRIDE + V_STRIDE);
  if (lds > 64 * 1024) {
    int dev = 0;
    TD_CHECK_HIP(hipGetDevice(&dev));
    if (!((done.load(std::memory_order_acquire) >> (dev & 63)) & 1ull)) {
      TD_CHECK_HIP(hipFuncSetAttribute((const void*)td_ip_attention_kernel<NP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      done.fetch_or(1ull << (dev & 63), std::memory_order_release);
    }
  }
  const int rows_wg = 64 * p.passes;
  const dim3 grid((unsigned)((p.rows + rows_wg - 1) / rows_wg), (unsigned)p.H);
  hipLaunchKernelGGL(td_ip_attention_kernel<NP>, grid, dim3(256), lds, s, p);
  TD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

int td_ip_attention_launch(const bf16_t* q, int ldq, const bf16_t* k, const bf16_t* v, int ldkv, bf16_t* o, int ldo, int rows, int H, int n_keys,
                           const bf16_t* norm_w, float eps, float out_scale, int accumulate, hipStream_t stream) {
  TD_CHECK_ARG(q && k && v && o, "td_ip_attention: null q / k / v / o");
  TD_CHECK_ARG(rows >= 1 && H >= 1 && H <= 65535, "td_ip_attention: rows=%d, H=%d (rows >= 1, 1 <= H <= 65535)", rows, H);
  TD_CHECK_ARG(n_keys >= 1 && n_keys <= TD_IP_MAX_KEYS, "td_ip_attention: n_keys=%d outside 1 .. %d (TD_IP_MAX_KEYS)", n_keys, TD_IP_MAX_KEYS);
  const long long w = (long long)H * 128;
  TD_CHECK_ARG(ldq >= w && ldq % 8 == 0, "td_ip_attention: ldq=%d must be a multiple of 8 and hold H x 128 = %lld columns", ldq, w);
  TD_CHECK_ARG(ldkv >= w && ldkv % 8 == 0, "td_ip_attention: ldkv=%d must be a multiple of 8 and hold H x 128 = %lld columns", ldkv, w);
  TD_CHECK_ARG(ldo >= w && ldo % 8 == 0, "td_ip_attention: ldo=%d must be a multiple of 8 and hold H x 128 = %lld columns", ldo, w);
  TD_CHECK_ARG((uintptr_t)q % 16 == 0, "td_ip_attention: q must be 16-byte aligned");
  TD_CHECK_ARG((uintptr_t)k % 16 == 0 && (uintptr_t)v % 16 == 0, "td_ip_attention: k and v must be 16-byte aligned");
  TD_CHECK_ARG((uintptr_t)o % 16 == 0, "td_ip_attention: o must be 16-byte aligned");
  TD_CHECK_ARG((uintptr_t)norm_w % 16 == 0, "td_ip_attention: norm_w must be 16-byte aligned");
  TD_CHECK_ARG(std::isfinite(out_scale), "td_ip_attention: out_scale is not finite");
  IpParams p{q, k, v, norm_w, o, rows, H, n_keys, ldq, ldkv, ldo, out_scale, eps, accumulate ? 1 : 0, 0};
  // rows per workgroup: enough to pay for staging the head's K and V, few enough to fill the chip at rows ~ 4096
  p.passes = n_keys <= 64 ? 2 : 4;
  if (n_keys <= 32) return launch_np<1>(p, stream);
  if (n_keys <= 64) return launch_np<2>(p, stream);
  if (n_keys <= 128) return launch_np<4>(p, stream);
  return launch_np<8>(p, stream);
}

extern "C" int td_ip_attention_bf16(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int64_t ldo, int rows, int H,
                                    int n_keys, const void* norm_w, float eps, float out_scale, int accumulate, void* stream) {
  TD_CHECK_ARG(ldq >= 0 && ldq < (1ll << 31) && ldkv >= 0 && ldkv < (1ll << 31) && ldo >= 0 && ldo < (1ll << 31),
               "td_ip_attention: ldq=%lld / ldkv=%lld / ldo=%lld outside the 32-bit range", (long long)ldq, (long long)ldkv, (long long)ldo);
  return td_ip_attention_launch((const bf16_t*)q, (int)ldq, (const bf16_t*)k, (const bf16_t*)v, (int)ldkv, (bf16_t*)o, (int)ldo, rows, H, n_keys,
                                (const bf16_t*)norm_w, eps, out_scale, accumulate, (hipStream_t)stream);
}
