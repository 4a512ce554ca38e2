// Pieces the two sampler kernels share (sampler.hip: td_sample_top_p_bf16; sampler_rows.hip: td_sample_rows_bf16): the workgroup shape, the
// counter-based generator behind the draw, and the workgroup prefix sum.  Both kernels must keep the same draw for the same (seed, offset, stream).
#pragma once
#include "td_common.h"

namespace td_sampler_detail {

constexpr int NT = 1024;            // threads per workgroup
constexpr int NW = NT / 64;         // waves
typedef unsigned long long u64;

__device__ __forceinline__ u64 splitmix64(u64 z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the 64 random bits of (seed, offset, stream): row r of td_sample_top_p_bf16 is stream r
__device__ __forceinline__ u64 draw_bits(u64 seed, u64 offset, u64 stream) {
  return splitmix64(splitmix64(seed ^ (0xD1B54A32D192ED03ull * (offset + 1ull))) ^ (0x9E3779B97F4A7C15ull * (stream + 1ull)));
}

// exclusive prefix sum of one value per thread over the workgroup (thread order); total in *tot.  `scratch`: NW + 1 slots.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* scratch, T* tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) scratch[w] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    T run = 0;
    for (int i = 0; i < NW; ++i) { const T t = scratch[i]; scratch[i] = run; run += t; }
    scratch[NW] = run;
  }
  __syncthreads();
  const T base = scratch[w];
  *tot = scratch[NW];
  __syncthreads();
  return base + inc - v;
}

}  // namespace td_sampler_detail
