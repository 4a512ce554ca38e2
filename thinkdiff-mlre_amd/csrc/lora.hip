// LoRA weight merge: w_out[n, k] = RNE_bf16( float(w_base[n, k]) + sum_i scale_i * sum_r B_i[n, r] * A_i[r, k] ).
//
// Replaces [ext] peft LoraLayer.merge / get_delta_weight (`weight + scaling * (lora_B.weight @ lora_A.weight)`) as diffusers' fuse_lora calls it,
// with two differences that make the merge a pure function of (base, adapters, weights): the update of ALL active adapters is summed in fp32 and
// added to an untouched base in fp32 with ONE rounding to bf16 (peft rounds the update to the weight's dtype, then adds, once per adapter).
//
// A streaming kernel: 2 B read + 2 B written per weight element, 2 * sum(rank) FLOP; the inner products run on v_mfma_f32_32x32x16_bf16.
// Orientation: the MFMA computes the TRANSPOSED update tile  D[k, n] = sum_r At[k, r] * Bt[r, n]  (MFMA "A" operand = lora_A transposed, MFMA "B"
// operand = lora_B transposed), because the 32x32 accumulator keeps its column on the lane and its rows in the registers: with k on the rows a lane
// owns runs of 4 consecutive k of ONE weight row n, and one half-swap (v_permlane32_swap) per register pair widens that to 8 consecutive k = one
// 16-byte load of the base and one 16-byte store of the result (the T21 form of the attention epilogue, done here on the fp32 accumulators so that
// the base is added before the only rounding).
//
// Operand layout ("packed", made once per adapter by td_lora_pack_bf16, never per merge): At [K, r_pad] = lora_A.weight transposed, then
// Bp [N, r_pad] = lora_B.weight, both with the rank zero-padded to r_pad = 16 * ceil(rank / 16), the k-extent of one MFMA: every fragment is one
// 16-byte contiguous read (lane (c, h) of k-step s: At[k0 + c][16 s + 8 h ..+8), Bp[n0 + c][16 s + 8 h ..+8)), and padded ranks multiply zeros.
//
// One wave per 32 (n) x 64 (k) tile of the weight, no LDS: the operands of a tile are (32 + 64) * r_pad * 2 bytes, re-read by the waves of the same
// row / column band out of L2 (a whole adapter pair of a 3072^2 Linear at rank 128 is 1.5 MB).
#include <cmath>

#include "td_kernels.h"
#include "../../include/thinkdiff_hip.h"

namespace {

constexpr int LORA_MAX = TD_LORA_MAX_ADAPTERS;

struct LoraOperands {
  const bf16_t* packed[LORA_MAX];   // At [K, r_pad] | Bp [N, r_pad]
  int r_pad[LORA_MAX];
  float scale[LORA_MAX];
  int n;
};

inline int pad16(int r) { return (r + 15) & ~15; }

}  // namespace

// one thread per packed element
__global__ void td_lora_pack_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B, int rank, int r_pad, int N, int K,
                                    bf16_t* __restrict__ packed) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nA = (long long)K * r_pad, nB = (long long)N * r_pad;
  if (i >= nA + nB) return;
  bf16_t v = 0;
  if (i < nA) {
    const int k = (int)(i / r_pad), r = (int)(i % r_pad);
    if (r < rank) v = A[(size_t)r * K + k];
  } else {
    const long long j = i - nA;
    const int n = (int)(j / r_pad), r = (int)(j % r_pad);
    if (r < rank) v = B[(size_t)n * rank + r];
  }
  packed[i] = v;
}

__global__ __launch_bounds__(256) void td_lora_merge_kernel(const bf16_t* w_base, bf16_t* w_out, int N, int K, LoraOperands op) {
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int tiles_k = K >> 6;
  const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n0 = (int)(tile / tiles_k) * 32, k0 = (int)(tile % tiles_k) * 64;
  if (n0 >= N) return;                       // (wave-uniform: the last block's spare waves)
  const int n = n0 + c;
  const bool row_ok = n < N;                 // N % 8 == 0: the last row band may be partial

  f32x16_t tot[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) tot[t][j] = 0.f;

  for (int i = 0; i < op.n; ++i) {
    const int rp = op.r_pad[i];
    const bf16_t* At = op.packed[i];
    const bf16_t* Bp = At + (size_t)K * rp;
    const bf16_t* a0 = At + (size_t)(k0 + c) * rp + 8 * h;
    const bf16_t* a1 = a0 + (size_t)32 * rp;
    const bf16_t* b = Bp + (size_t)(row_ok ? n : n0) * rp + 8 * h;      // rows past N: a valid address, the result is never stored
    f32x16_t acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
    for (int s = 0; s < rp; s += 16) {
      const bf16x8_t fb = *(const bf16x8_t*)(b + s);
      const bf16x8_t fa0 = *(const bf16x8_t*)(a0 + s);
      const bf16x8_t fa1 = *(const bf16x8_t*)(a1 + s);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0, fb, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1, fb, acc[1], 0, 0, 0);
    }
    const float sc = op.scale[i];             // on the fp32 sum of THIS adapter, never inside a bf16 operand
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) tot[t][j] += sc * acc[t][j];
  }

  // accumulator (t, reg 4 g + j) of lane (c, h) = update[n0 + c][k0 + 32 t + 8 g + 4 h + j].  Per pair of groups (g, g + 1), g even: the upper lanes'
  // group g goes down, the lower lanes' group g + 1 up -- then lane (c, h) owns the 8 consecutive k from k0 + 32 t + 8 (g + h).
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      float u[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const auto r = __builtin_amdgcn_permlane32_swap(as_u32(tot[t][4 * g + j]), as_u32(tot[t][4 * (g + 1) + j]), false, false);
        u[j] = as_f32(r[0]);
        u[4 + j] = as_f32(r[1]);
      }
      if (row_ok) {
        const size_t off = (size_t)n * K + k0 + 32 * t + 8 * (g + h);
        const u32x4_t w = *(const u32x4_t*)(w_base + off);
        u32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack_bf2(bf_lo(w[j]) + u[2 * j], bf_hi(w[j]) + u[2 * j + 1]);
        *(u32x4_t*)(w_out + off) = o;
      }
    }
}

extern "C" {

size_t td_lora_packed_bytes(int rank, int N, int K) {
  if (rank < 1 || N < 1 || K < 1) return 0;
  return (size_t)((long long)N + K) * pad16(rank) * sizeof(bf16_t);
}

int td_lora_pack_bf16(const void* A, const void* B, int rank, int N, int K, void* packed, void* stream) {
  TD_CHECK_ARG(A && B && packed, "td_lora_pack_bf16: null argument");
  TD_CHECK_ARG(rank >= 1, "td_lora_pack_bf16: rank=%d must be at least 1", rank);
  TD_CHECK_ARG(N > 0 && K > 0 && K % 64 == 0 && N % 8 == 0, "td_lora_pack_bf16: N=%d must be a positive multiple of 8, K=%d of 64", N, K);
  TD_CHECK_ARG((uintptr_t)packed % 16 == 0, "td_lora_pack_bf16: packed must be 16-byte aligned");
  const int rp = pad16(rank);
  TD_GRID_1D(blocks, ((long long)N + K) * rp, 256, "td_lora_pack_bf16");
  hipLaunchKernelGGL(td_lora_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)A, (const bf16_t*)B, rank, rp, N, K,
                     (bf16_t*)packed);
  TD_CHECK_LAUNCH();
  return TD_OK;
}

int td_lora_merge_bf16(const void* w_base, void* w_out, int N, int K, int n_adapters, const void* const* packed, const int* ranks,
                       const float* scales, void* stream) {
  TD_CHECK_ARG(w_base && w_out, "td_lora_merge_bf16: null weight pointer");
  TD_CHECK_ARG(n_adapters >= 0 && n_adapters <= LORA_MAX, "td_lora_merge_bf16: %d adapters, one call takes at most %d", n_adapters, LORA_MAX);
  TD_CHECK_ARG(n_adapters == 0 || (packed && ranks && scales), "td_lora_merge_bf16: null adapter arrays with %d adapters", n_adapters);
  TD_CHECK_ARG(N > 0 && K > 0 && K % 64 == 0 && N % 8 == 0, "td_lora_merge_bf16: N=%d must be a positive multiple of 8, K=%d of 64", N, K);
  TD_CHECK_ARG((uintptr_t)w_base % 16 == 0 && (uintptr_t)w_out % 16 == 0, "td_lora_merge_bf16: w_base / w_out must be 16-byte aligned");
  LoraOperands op;
  op.n = 0;
  for (int i = 0; i < n_adapters; ++i) {
    TD_CHECK_ARG(packed[i], "td_lora_merge_bf16: adapter %d: null operands", i);
    TD_CHECK_ARG((uintptr_t)packed[i] % 16 == 0, "td_lora_merge_bf16: adapter %d: operands must be 16-byte aligned", i);
    TD_CHECK_ARG(ranks[i] >= 1, "td_lora_merge_bf16: adapter %d: rank=%d must be at least 1", i, ranks[i]);
    TD_CHECK_ARG(std::isfinite(scales[i]), "td_lora_merge_bf16: adapter %d: scale is not finite", i);
    if (scales[i] == 0.f) continue;          // contributes nothing, whatever its operands hold
    op.packed[op.n] = (const bf16_t*)packed[i];
    op.r_pad[op.n] = pad16(ranks[i]);
    op.scale[op.n] = scales[i];
    ++op.n;
  }
  if (op.n == 0) {                           // the base bits (the kernel's w + 0.0f would turn a -0 weight into +0)
    if (w_out != w_base) TD_CHECK_HIP(hipMemcpyAsync(w_out, w_base, (size_t)N * K * sizeof(bf16_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TD_OK;
  }
  const long long tiles = (long long)((N + 31) / 32) * (K / 64);
  TD_GRID_1D(blocks, (tiles + 3) / 4 * 256, 256, "td_lora_merge_bf16");
  hipLaunchKernelGGL(td_lora_merge_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w_base, (bf16_t*)w_out, N, K, op);
  TD_CHECK_LAUNCH();
  return TD_OK;
}

}  // extern "C"
