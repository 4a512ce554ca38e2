// FLUX.1 Redux: several [text | image] prompt streams folded into one ([ext] diffusers FluxPriorReduxPipeline.__call__, restated:
//   prompt_embeds = cat([text, image_embeds], dim=1);  prompt_embeds *= scale[:, None, None];  prompt_embeds = sum(prompt_embeds, dim=0, keepdim=True)
// on bf16 tensors).  One memory-bound row kernel, 16 B per lane, no concatenated intermediate:
//
//   out[r, :]     = bf16( sum_b float( bf16( s_b * text[b, r, :] ) ) )        r < T          (text null: +0.0, nothing read)
//   out[T + r, :] = bf16( sum_b float( bf16( s_b * image[b, r, :] ) ) )       r < S
//
// The rounding points are those of the two torch statements: s_b is the scale rounded to bf16 (by the launcher, on the host), every product is
// rounded to bf16 (a product of two bf16 values is exact in fp32, so this is ONE rounding), the sum runs in fp32 in index order b = 0, 1, ..
// starting FROM the b = 0 term (B = 1 with scale 1 returns the input's bits, a negative zero included), and is rounded once.
#include <cmath>
#include <cstring>
#include "td_kernels.h"

namespace {

constexpr int RX_THREADS = 256, RX_MAX_STREAMS = 16;

struct ReduxScales { float s[RX_MAX_STREAMS]; };      // bf16-representable values; travels in the kernel's argument segment

__global__ __launch_bounds__(RX_THREADS) void td_redux_compose_kernel(const bf16_t* text, long long text_bs, int T, const bf16_t* image, long long image_bs,
                                                                       ReduxScales sc, int B, int D, bf16_t* out, int ldo, int total, int chunks) {
  const int idx = blockIdx.x * RX_THREADS + threadIdx.x;      // (total < 2^31: the launcher checks)
  if (idx >= total) return;
  const int r = idx / chunks, c = idx - r * chunks;
  bf16_t* dst = out + (size_t)r * ldo + c * 8;
  const bf16_t* src;
  long long bs;
  if (r < T) {
    if (!text) { *(u32x4_t*)dst = u32x4_t{0u, 0u, 0u, 0u}; return; }
    src = text + (size_t)r * D + c * 8; bs = text_bs;
  } else {
    src = image + (size_t)(r - T) * D + c * 8; bs = image_bs;
  }
  float acc[8];
#pragma unroll 1
  for (int b = 0; b < B; ++b) {
    const u32x4_t v = *(const u32x4_t*)(src + b * bs);
    const float s = sc.s[b];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float lo = rbf(s * bf_lo(v[i])), hi = rbf(s * bf_hi(v[i]));
      if (b == 0) { acc[2 * i] = lo; acc[2 * i + 1] = hi; }
      else { acc[2 * i] += lo; acc[2 * i + 1] += hi; }
    }
  }
  u32x4_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = pack_bf2(acc[2 * i], acc[2 * i + 1]);
  *(u32x4_t*)dst = o;
}

// float -> the nearest bf16 (ties to even), back as a float: torch's `tensor(scale, dtype=bfloat16)`
float round_bf16_host(float f) {
  if (std::isnan(f)) return f;
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  std::memcpy(&f, &u, 4);
  return f;
}

}  // namespace

int td_redux_compose_launch(const bf16_t* text, long long text_bstride, int T, const bf16_t* image, long long image_bstride, int S, const float* scales,
                            int B, int D, bf16_t* out, long long ldo, hipStream_t stream) {
  TD_CHECK_ARG(D > 0 && D % 8 == 0, "td_redux_compose: D=%d must be a positive multiple of 8", D);
  TD_CHECK_ARG(B >= 1 && B <= RX_MAX_STREAMS, "td_redux_compose: B=%d streams, 1 .. %d are supported", B, RX_MAX_STREAMS);
  TD_CHECK_ARG(T >= 0 && S >= 0 && (long long)T + S > 0, "td_redux_compose: T=%d, S=%d: both must be non-negative and T + S positive", T, S);
  TD_CHECK_ARG(ldo >= D && ldo % 8 == 0, "td_redux_compose: ldo=%lld must be a multiple of 8 and at least D=%d", ldo, D);
  TD_CHECK_ARG(image || S == 0, "td_redux_compose: image is null with S=%d rows", S);
  TD_CHECK_ARG(scales, "td_redux_compose: scales is null (B host floats)");
  TD_CHECK_ARG(out, "td_redux_compose: out is null");
  TD_CHECK_ARG(text_bstride >= 0 && image_bstride >= 0 && text_bstride % 8 == 0 && image_bstride % 8 == 0,
               "td_redux_compose: text_bstride=%lld / image_bstride=%lld must be non-negative multiples of 8", text_bstride, image_bstride);
  TD_CHECK_ARG(((uintptr_t)text | (uintptr_t)image | (uintptr_t)out) % 16 == 0, "td_redux_compose: text, image and out must be 16-byte aligned");
  const long long rows = (long long)T + S;
  TD_CHECK_ARG(rows * D <= 0x7fffffffll, "td_redux_compose: (T + S) x D = %lld x %d elements exceed the kernel's 32-bit index", rows, D);
  TD_CHECK_ARG(ldo < (1ll << 31), "td_redux_compose: ldo=%lld outside the 32-bit range", ldo);
  ReduxScales sc = {};
  for (int b = 0; b < B; ++b) sc.s[b] = round_bf16_host(scales[b]);
  TD_GRID_1D_I32(nblk, rows * (D / 8), RX_THREADS, "td_redux_compose");
  hipLaunchKernelGGL(td_redux_compose_kernel, dim3(nblk), dim3(RX_THREADS), 0, stream, text, text_bstride, T, image, image_bstride, sc, B, D, out, (int)ldo,
                     (int)(rows * (D / 8)), D / 8);
  TD_CHECK_LAUNCH();
  return 0;
}
