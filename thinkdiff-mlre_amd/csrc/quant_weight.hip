// Weight-only 8-bit quantisation for the skinny-M weight streams (csrc/gemv_bf16.hip, W8 forms): the e4m3 power-of-two format of csrc/e4m3_pow2.h with
// one scale per output row of a Linear weight W[N, K].  Runs once per load (not hot); one workgroup per row, the row maximum through shuffles and LDS
// (a maximum does not depend on the order it is taken in).  Further down: the MXFP4 twin, and the grouped int4 format of csrc/int4_group.h, which is not
// quantised here but repacked from AWQ / GPTQ checkpoint tensors.
#include "td_common.h"
#include "td_kernels.h"
#include "e4m3_pow2.h"
#include "mxfp4_pow2.h"
#include "int4_group.h"

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

// Grouped int4 (csrc/int4_group.h) from a checkpoint Linear, one launch.  A thread owns 8 output rows (n = 8c .. 8c + 7) x one unit of 8 k (u): the 64
// nibbles arrive in 8 dwords -- AWQ: qweight[8u + i, c], one per k, each holding the 8 rows in AutoAWQ's interleave; GPTQ: qweight[u, 8c + j], one per row,
// each holding the 8 k in order -- and leave as one dword per row.  c runs fastest over the threads, so the reads are coalesced and the 4-byte writes are
// not (once per Linear at load).  The first K / G units of a column block also carry its groups: thread (c, u = g) moves the 8 scales and zero points
// of group g.  gptq_v1: the checkpoint stores z - 1 (AutoGPTQ's own unpack adds the 1 back, modulo 16).
__global__ __launch_bounds__(QW_THREADS) void td_repack_int4_kernel(bool awq, bool gptq_v1, const unsigned* qweight, const unsigned* qzeros, const uint16_t* scales_in,
                                                                    int N, int K, int ngroups, unsigned* packed, uint16_t* scales, uint8_t* zeros) {
  const int NC = N >> 3, NU = K >> 3;
  const long long idx = (long long)blockIdx.x * QW_THREADS + threadIdx.x;
  if (idx >= (long long)NC * NU) return;
  const int c = (int)(idx % NC), u = (int)(idx / NC);
  unsigned in[8], out[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) in[i] = awq ? qweight[(size_t)(8 * u + i) * NC + c] : qweight[(size_t)u * N + 8 * c + i];
#pragma unroll
  for (int j = 0; j < 8; ++j)        // row 8c + j
#pragma unroll
    for (int i = 0; i < 8; ++i) {    // k = 8u + i
      const unsigned q = awq ? in[i] >> (4 * ((j >> 1) + 4 * (j & 1))) : in[j] >> (4 * i);
      out[j] |= i4_place(q, i);
    }
#pragma unroll
  for (int j = 0; j < 8; ++j) packed[(size_t)(8 * c + j) * NU + u] = out[j];
  if (u >= ngroups) return;
  const unsigned zw = qzeros[(size_t)u * NC + c];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned z = awq ? zw >> (4 * ((j >> 1) + 4 * (j & 1))) : (zw >> (4 * j)) + (gptq_v1 ? 1u : 0u);
    zeros[(size_t)(8 * c + j) * ngroups + u] = (uint8_t)(z & 15u);
    scales[(size_t)(8 * c + j) * ngroups + u] = scales_in[(size_t)u * N + 8 * c + j];
  }
}

__global__ __launch_bounds__(QW_THREADS) void td_dequant_rows_int4_kernel(const uint8_t* packed, const uint16_t* scales, const uint8_t* zeros, int gshift, bf16_t* w_hat,
                                                                          long long ldw, int K) {
  const int n = blockIdx.x;
  const unsigned* sq = (const unsigned*)(packed + (size_t)n * (K >> 1));
  const uint16_t* ss = scales + (size_t)n * (K >> gshift);
  const uint8_t* sz = zeros + (size_t)n * (K >> gshift);
  u32x4_t* dh = (u32x4_t*)(w_hat + (size_t)n * ldw);
  for (int c = threadIdx.x; c < (K >> 3); c += QW_THREADS) {
    const int g = (8 * c) >> gshift;
    dh[c] = i4_to_bf16(sq[c], i4_group(ss[g], sz[g]));
  }
}

// the shape rules every grouped-int4 entry shares (`me`: the entry's name at the C ABI)
int int4_shape_check(const char* me, int N, int K, int G) {
  TD_CHECK_ARG(i4_gshift_of(G) != 0, "%s: G=%d: the group sizes served are 32, 64 and 128", me, G);
  TD_CHECK_ARG(N > 0 && K > 0 && K % G == 0 && K % I4_CHUNK == 0, "%s: N=%d, K=%d: K must be a multiple of G=%d and of 32 (one 16-byte chunk of a packed row)", me, N, K, G);
  return 0;
}

}  // namespace

int td_repack_int4_launch(int layout, const int* qweight, const int* qzeros, const uint16_t* scales_in, const int* g_idx, int N, int K, int G, uint8_t* packed,
                          uint16_t* scales, uint8_t* zeros, hipStream_t stream) {
  (void)g_idx;      // only the trivial map k / G is served (no act-order): the caller vouches for it
  TD_CHECK_ARG(layout == 0 || layout == 1 || layout == 3, "td_repack_int4: layout=%d: TD_INT4_AWQ = 0, TD_INT4_GPTQ = 1 and TD_INT4_GPTQ | TD_INT4_GPTQ_V2 = 3 are the ones served", layout);
  TD_CHECK_ARG(qweight && qzeros && scales_in, "td_repack_int4: qweight, qzeros and scales_in are required");
  TD_CHECK_ARG(packed && scales && zeros, "td_repack_int4: packed, scales and zeros are required");
  if (int rc = int4_shape_check("td_repack_int4", N, K, G)) return rc;
  TD_CHECK_ARG(N % 8 == 0, "td_repack_int4: N=%d must be a multiple of 8 (the checkpoint packs 8 output rows, or their zero points, into an int32)", N);
  TD_CHECK_ARG(((uintptr_t)qweight | (uintptr_t)qzeros | (uintptr_t)packed) % 4 == 0 && ((uintptr_t)scales_in | (uintptr_t)scales) % 2 == 0,
               "td_repack_int4: misaligned operands: qweight, qzeros and packed must be 4-byte aligned, scales_in and scales 2-byte");
  const long long threads = (long long)(N / 8) * (K / 8);
  hipLaunchKernelGGL(td_repack_int4_kernel, dim3((unsigned)((threads + QW_THREADS - 1) / QW_THREADS)), dim3(QW_THREADS), 0, stream, layout == 0, layout == 1,
                     (const unsigned*)qweight, (const unsigned*)qzeros, scales_in, N, K, K / G, (unsigned*)packed, scales, zeros);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_dequant_rows_int4_launch(const uint8_t* packed, const uint16_t* scales, const uint8_t* zeros, int G, bf16_t* w_hat, long long ldw, int N, int K, hipStream_t stream) {
  TD_CHECK_ARG(packed && scales && zeros, "td_dequant_rows_int4: packed, scales and zeros are required");
  TD_CHECK_ARG(w_hat, "td_dequant_rows_int4: w_hat is required");
  if (int rc = int4_shape_check("td_dequant_rows_int4", N, K, G)) return rc;
  TD_CHECK_ARG(ldw >= K && ldw % 8 == 0 && ldw < (1ll << 31), "td_dequant_rows_int4: ldw=%lld must be a multiple of 8, at least K and below 2^31", ldw);
  TD_CHECK_ARG((uintptr_t)w_hat % 16 == 0 && (uintptr_t)packed % 4 == 0 && (uintptr_t)scales % 2 == 0,
               "td_dequant_rows_int4: misaligned rows: w_hat must be 16-byte aligned, packed 4-byte, scales 2-byte");
  hipLaunchKernelGGL(td_dequant_rows_int4_kernel, dim3((unsigned)N), dim3(QW_THREADS), 0, stream, packed, scales, zeros, i4_gshift_of(G), w_hat, ldw, K);
  TD_CHECK_LAUNCH();
  return 0;
}

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
