// First-block cache of the FLUX denoise loop ([ext] diffusers hooks/first_block_cache.py, restated; the engine side is run_blocks in
// csrc/flux_engine.hip).  Two memory-bound row kernels over bf16 rows of D columns at their own leading dimensions, 16 B per lane:
//
//   td_block_cache_head:  r = bf16(float(h1) - float(h0))          the first block's residual of THIS forward
//                         sums[0] = sum |r - r_prev|,  sums[1] = sum |r_prev|          (r_prev null: both terms skipped, sums[1] = 0)
//   td_block_cache_tail:  out = bf16(float(a) - float(b))          what the remaining blocks added (out may be a or b: in place)
//
// The sums decide whether a forward runs its remaining blocks, and images in flight must take the decisions of sequential runs: the
// reduction uses no atomics and has ONE combination order, fixed by (rows, D) alone -- never by the device, the occupancy or what else runs.
//   thread:  fp32 sum of its terms in index order (grid-stride; at most a few dozen terms at FLUX sizes)
//   wave:    xor-butterfly over 64 lanes in fp64;   block: its 4 waves in order, fp64 -> partials[block]
//   finish:  one workgroup; thread t adds partials t, t + 256, .. in order, then the same butterfly and wave order -> sums (fp64)
// The grid is min(ceil(chunks / 1024), 4096) workgroups: 9216 x 3072 elements give 54 fp32 terms per thread, everything above them is fp64.
#include "td_kernels.h"

namespace {

constexpr int BC_THREADS = 256, BC_MAX_BLOCKS = 4096, BC_CHUNKS_PER_THREAD = 4;

__device__ __forceinline__ void unpack8(const u32x4_t v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = bf_lo(v[i]);
    f[2 * i + 1] = bf_hi(v[i]);
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (a, b) of every thread -> the block's sums in thread 0: butterfly per wave, then the waves in order
__device__ __forceinline__ void block_sum2(double& a, double& b) {
  __shared__ double part[BC_THREADS / 64][2];
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[w][0] = a; part[w][1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = part[0][0]; b = part[0][1];
#pragma unroll
    for (int i = 1; i < BC_THREADS / 64; ++i) { a += part[i][0]; b += part[i][1]; }
  }
}

__global__ __launch_bounds__(BC_THREADS) void td_block_cache_head_kernel(const bf16_t* h1, int ld1, const bf16_t* h0, int ld0, const bf16_t* rp, int ldp,
                                                                          bf16_t* r, int ldr, int total, int chunks, double* partials) {
  float num = 0.f, den = 0.f;
  for (int idx = blockIdx.x * BC_THREADS + threadIdx.x; idx < total; idx += gridDim.x * BC_THREADS) {      // (total < 2^31 - grid x block: the launcher checks)
    const int m = idx / chunks, c = idx - m * chunks;
    float a[8], b[8];
    unpack8(*(const u32x4_t*)(h1 + (size_t)m * ld1 + c * 8), a);
    unpack8(*(const u32x4_t*)(h0 + (size_t)m * ld0 + c * 8), b);
    u32x4_t out;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = pack_bf2(a[2 * i] - b[2 * i], a[2 * i + 1] - b[2 * i + 1]);
    *(u32x4_t*)(r + (size_t)m * ldr + c * 8) = out;
    if (rp) {      // the metric reads the ROUNDED residual, as the tensors diffusers compares are
      float x[8], p[8];
      unpack8(out, x);
      unpack8(*(const u32x4_t*)(rp + (size_t)m * ldp + c * 8), p);
#pragma unroll
      for (int i = 0; i < 8; ++i) { num += fabsf(x[i] - p[i]); den += fabsf(p[i]); }
    }
  }
  double dn = num, dd = den;
  block_sum2(dn, dd);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = dn; partials[2 * blockIdx.x + 1] = dd; }
}

__global__ __launch_bounds__(BC_THREADS) void td_block_cache_finish_kernel(const double* partials, int n, double* sums) {
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n; i += BC_THREADS) { a += partials[2 * i]; b += partials[2 * i + 1]; }
  block_sum2(a, b);
  if (threadIdx.x == 0) { sums[0] = a; sums[1] = b; }
}

__global__ __launch_bounds__(BC_THREADS) void td_block_cache_tail_kernel(const bf16_t* a, int lda, const bf16_t* b, int ldb, bf16_t* out, int ldo, int total, int chunks) {
  const int idx = blockIdx.x * BC_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int m = idx / chunks, c = idx - m * chunks;
  float x[8], y[8];
  unpack8(*(const u32x4_t*)(a + (size_t)m * lda + c * 8), x);
  unpack8(*(const u32x4_t*)(b + (size_t)m * ldb + c * 8), y);
  u32x4_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = pack_bf2(x[2 * i] - y[2 * i], x[2 * i + 1] - y[2 * i + 1]);
  *(u32x4_t*)(out + (size_t)m * ldo + c * 8) = o;      // (in place on a or b: every lane has read its own 16 bytes)
}

// the bytes rows of D columns at stride ld span
struct Extent { uintptr_t lo, hi; };
Extent extent(const void* p, int ld, int rows, int D) { return {(uintptr_t)p, (uintptr_t)p + ((uintptr_t)(rows - 1) * ld + D) * sizeof(bf16_t)}; }
bool disjoint(Extent a, Extent b) { return a.lo >= b.hi || b.lo >= a.hi; }

}  // namespace

int td_block_cache_head_launch(const bf16_t* h1, int ld1, const bf16_t* h0, int ld0, const bf16_t* r_prev, int ldp, bf16_t* r, int ldr, int rows, int D,
                               double* sums, double* ws, hipStream_t stream) {
  TD_CHECK_ARG(h1 && h0 && r && sums && ws, "td_block_cache_head: null argument (only r_prev may be null: no previous residual)");
  TD_CHECK_ARG(rows > 0 && D > 0 && D % 8 == 0, "td_block_cache_head: rows=%d, D=%d: D must be a positive multiple of 8, rows positive", rows, D);
  TD_CHECK_ARG(ld1 % 8 == 0 && ld0 % 8 == 0 && ldr % 8 == 0 && ld1 >= D && ld0 >= D && ldr >= D && (!r_prev || (ldp % 8 == 0 && ldp >= D)),
               "td_block_cache_head: leading dimensions %d / %d / %d / %d must be multiples of 8 and at least D=%d", ld1, ld0, ldp, ldr, D);
  TD_CHECK_ARG(((uintptr_t)h1 | (uintptr_t)h0 | (uintptr_t)r_prev | (uintptr_t)r) % 16 == 0 && ((uintptr_t)sums | (uintptr_t)ws) % 8 == 0,
               "td_block_cache_head: the row buffers must be 16-byte aligned, sums and the workspace 8-byte");
  const Extent er = extent(r, ldr, rows, D);
  TD_CHECK_ARG(disjoint(er, extent(h1, ld1, rows, D)) && disjoint(er, extent(h0, ld0, rows, D)) && (!r_prev || disjoint(er, extent(r_prev, ldp, rows, D))),
               "td_block_cache_head: r must not overlap h1, h0 or r_prev");
  const long long total = (long long)rows * (D / 8);
  long long nblk = (total + BC_THREADS * BC_CHUNKS_PER_THREAD - 1) / (BC_THREADS * BC_CHUNKS_PER_THREAD);
  if (nblk > BC_MAX_BLOCKS) nblk = BC_MAX_BLOCKS;
  TD_CHECK_ARG(total + nblk * BC_THREADS < (1ll << 31), "td_block_cache_head: %lld work-items exceed the kernel's 32-bit index", total);
  hipLaunchKernelGGL(td_block_cache_head_kernel, dim3((unsigned)nblk), dim3(BC_THREADS), 0, stream, h1, ld1, h0, ld0, r_prev, ldp, r, ldr, (int)total, D / 8, ws);
  TD_CHECK_LAUNCH();
  hipLaunchKernelGGL(td_block_cache_finish_kernel, dim3(1), dim3(BC_THREADS), 0, stream, (const double*)ws, (int)nblk, sums);
  TD_CHECK_LAUNCH();
  return 0;
}

int td_block_cache_tail_launch(const bf16_t* a, int lda, const bf16_t* b, int ldb, bf16_t* out, int ldo, int rows, int D, hipStream_t stream) {
  TD_CHECK_ARG(a && b && out, "td_block_cache_tail: null argument");
  TD_CHECK_ARG(rows > 0 && D > 0 && D % 8 == 0, "td_block_cache_tail: rows=%d, D=%d: D must be a positive multiple of 8, rows positive", rows, D);
  TD_CHECK_ARG(lda % 8 == 0 && ldb % 8 == 0 && ldo % 8 == 0 && lda >= D && ldb >= D && ldo >= D,
               "td_block_cache_tail: lda=%d, ldb=%d, ldo=%d must be multiples of 8 and at least D=%d", lda, ldb, ldo, D);
  TD_CHECK_ARG(((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) % 16 == 0, "td_block_cache_tail: the buffers must be 16-byte aligned");
  const Extent eo = extent(out, ldo, rows, D);
  TD_CHECK_ARG((disjoint(eo, extent(a, lda, rows, D)) || (out == a && ldo == lda)) && (disjoint(eo, extent(b, ldb, rows, D)) || (out == b && ldo == ldb)),
               "td_block_cache_tail: out may be a or b themselves (same leading dimension), not a shifted overlap of them");
  TD_GRID_1D_I32(nblk, (long long)rows * (D / 8), BC_THREADS, "td_block_cache_tail");
  hipLaunchKernelGGL(td_block_cache_tail_kernel, dim3(nblk), dim3(BC_THREADS), 0, stream, a, lda, b, ldb, out, ldo, (int)((long long)rows * (D / 8)), D / 8);
  TD_CHECK_LAUNCH();
  return 0;
}
