// PIL-exact separable image resize on uint8 HWC images (td_resize_coeffs, td_image_resize_u8) and the per-channel table
// lookup that follows it in the image processors (td_image_lut_chw_f32).
//
// [ext] Pillow src/libImaging/Resample.c: ImagingResample makes one coefficient table per axis (precompute_coeffs, double), turns
// it into 22-bit fixed point (normalize_coeffs_8bpc) and runs a horizontal pass, then a vertical pass over the horizontal pass's
// uint8 output; each output is clip8((2^21 + sum pixel * weight) >> 22).  After the tables everything is integer arithmetic, so
// the kernels below give Pillow's bytes, not an approximation of them.  The tables are made on the host: lanczos goes through
// libm's sin, which the device's sin does not reproduce bit for bit.
#include <math.h>
#include "td_kernels.h"

namespace {

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;      // Pillow's PRECISION_BITS: 8 bits of pixel, 2 bits of headroom for the overshoot of bicubic / lanczos
constexpr int RS_THREADS = 256;

// ---- the filters, as Pillow writes them (double) -------------------------------------------------------------------
#pragma clang fp contract(off)      // Pillow's doubles, operation by operation: no fused multiply-add, here and in td_resize_coeffs_host
double rs_bilinear(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}
double rs_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double rs_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double rs_lanczos(double x) {
  if (-3.0 <= x && x < 3.0) return rs_sinc(x) * rs_sinc(x / 3);
  return 0.0;
}

__device__ __forceinline__ unsigned char rs_clip8(int acc) {
  const int v = acc >> RS_PRECISION_BITS;      // arithmetic shift, as Pillow's clip8 on a signed int
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One thread per output byte, one output row per group of `chunks` workgroups, so the row index is uniform in a workgroup: in the vertical
// pass the window and its weights then come through scalar loads, shared by the whole wave.  Bytes are taken in memory order: a wave writes 64
// consecutive bytes and, for one window step, reads 64 consecutive source bytes (vertical pass: the same columns one row further) or bytes
// `scale` pixels apart whose windows overlap their neighbours' (horizontal pass: every source line is reused from L1 / L2 by the 2 * support
// neighbouring outputs).  The window loop has no fixed bound: count <= ksize, and ksize grows with the downscale factor (600 -> 28 lanczos: 131).
// src [rows, in_w, in_c] -> dst [rows, out_w, out_c]; grid = rows * chunks, chunks = ceil(out_w * out_c / RS_THREADS)
__global__ __launch_bounds__(RS_THREADS) void td_resize_h_kernel(const unsigned char* __restrict__ src, int in_w, int in_c, unsigned char* __restrict__ dst, int out_w,
                                                                 int out_c, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int chunks) {
  const int y = blockIdx.x / chunks;
  const int j = (blockIdx.x % chunks) * RS_THREADS + threadIdx.x;      // byte within the output row
  const int n_row = out_w * out_c;
  if (j >= n_row) return;
  const int c = j % out_c, xo = j / out_c;
  const int sc = in_c == 1 ? 0 : c;              // "L" replicated; "RGBA": the first three of four
  int xmin = bounds[2 * xo], cnt = bounds[2 * xo + 1];
  xmin = max(xmin, 0);                           // a table from td_resize_coeffs never needs these three; a foreign one cannot read past the row
  cnt = min(min(cnt, ksize), in_w - xmin);
  const int* k = kk + (size_t)xo * ksize;
  const unsigned char* s = src + ((size_t)y * in_w + xmin) * in_c + sc;
  int acc = 1 << (RS_PRECISION_BITS - 1);
  for (int i = 0; i < cnt; ++i) acc += (int)s[(size_t)i * in_c] * k[i];
  dst[(size_t)y * n_row + j] = rs_clip8(acc);
}

// src [in_h, w, in_c] -> dst [out_h, w, out_c]; grid = out_h * chunks, chunks = ceil(w * out_c / RS_THREADS)
__global__ __launch_bounds__(RS_THREADS) void td_resize_v_kernel(const unsigned char* __restrict__ src, int in_h, int w, int in_c, unsigned char* __restrict__ dst,
                                                                 int out_c, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int chunks) {
  const int yo = blockIdx.x / chunks;
  const int j = (blockIdx.x % chunks) * RS_THREADS + threadIdx.x;      // byte within the output row
  const int n_row = w * out_c;
  if (j >= n_row) return;
  const int c = j % out_c, x = j / out_c;
  const int sc = in_c == 1 ? 0 : c;
  int ymin = bounds[2 * yo], cnt = bounds[2 * yo + 1];
  ymin = max(ymin, 0);
  cnt = min(min(cnt, ksize), in_h - ymin);
  const int* k = kk + (size_t)yo * ksize;
  const size_t step = (size_t)w * in_c;
  const unsigned char* s = src + ((size_t)ymin * w + x) * in_c + sc;
  int acc = 1 << (RS_PRECISION_BITS - 1);
  for (int i = 0; i < cnt; ++i) acc += (int)s[i * step] * k[i];
  dst[(size_t)yo * n_row + j] = rs_clip8(acc);
}

// neither axis changes: a copy, or the channel conversion alone; n = h * w * out_c
__global__ __launch_bounds__(RS_THREADS) void td_resize_copy_kernel(const unsigned char* __restrict__ src, int in_c, unsigned char* __restrict__ dst, int out_c, int n) {
  const int idx = blockIdx.x * RS_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int c = idx % out_c, px = idx / out_c;
  dst[idx] = src[(size_t)px * in_c + (in_c == 1 ? 0 : c)];
}

// img uint8 [H, W, C] -> out fp32 [C, H, W], out[c, y, x] = lut[c, img[y, x, c]]; one thread per output element, n = C * H * W
__global__ __launch_bounds__(RS_THREADS) void td_image_lut_chw_kernel(const unsigned char* __restrict__ img, int hw, int C, const float* __restrict__ lut,
                                                                      float* __restrict__ out, int n) {
  const int idx = blockIdx.x * RS_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int c = idx / hw, p = idx % hw;
  out[idx] = lut[c * 256 + img[(size_t)p * C + c]];
}

}  // namespace

int td_resize_coeffs_host(int in_size, int out_size, int filter, int* bounds, int* kk, int* ksize_out) {
  TD_CHECK_ARG(in_size > 0, "td_resize_coeffs: in_size=%d must be positive", in_size);
  TD_CHECK_ARG(out_size > 0, "td_resize_coeffs: out_size=%d must be positive", out_size);
  double (*f)(double) = nullptr;
  double fsupport = 0.0;
  switch (filter) {
    case 1: f = rs_lanczos; fsupport = 3.0; break;
    case 2: f = rs_bilinear; fsupport = 1.0; break;
    case 3: f = rs_bicubic; fsupport = 2.0; break;
    case 0: TD_CHECK_ARG(false, "td_resize_coeffs: filter=0 (NEAREST) is not built; 1 = LANCZOS, 2 = BILINEAR, 3 = BICUBIC are"); break;
    case 4: TD_CHECK_ARG(false, "td_resize_coeffs: filter=4 (BOX) is not built; 1 = LANCZOS, 2 = BILINEAR, 3 = BICUBIC are"); break;
    case 5: TD_CHECK_ARG(false, "td_resize_coeffs: filter=5 (HAMMING) is not built; 1 = LANCZOS, 2 = BILINEAR, 3 = BICUBIC are"); break;
    default: TD_CHECK_ARG(false, "td_resize_coeffs: filter=%d is not a Pillow resampling code; 1 = LANCZOS, 2 = BILINEAR, 3 = BICUBIC are built", filter);
  }
  TD_CHECK_ARG(ksize_out, "td_resize_coeffs: ksize is null");
  TD_CHECK_ARG((bounds == nullptr) == (kk == nullptr), "td_resize_coeffs: bounds and kk must both be given, or both be null to query ksize");
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = fsupport * filterscale;
  TD_CHECK_ARG(support < (double)(1 << 28), "td_resize_coeffs: in_size=%d -> out_size=%d needs a window of %.0f taps, outside the 32-bit range", in_size, out_size, 2 * support);
  const int ksize = (int)ceil(support) * 2 + 1;
  TD_CHECK_ARG((long long)out_size * ksize < (1ll << 31), "td_resize_coeffs: out_size=%d x ksize=%d table entries are outside the 32-bit range", out_size, ksize);
  *ksize_out = ksize;
  if (!bounds) return 0;
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    // the weights are evaluated twice (sum, then value) so that no scratch array is needed; both evaluations give the same doubles
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += f((x + xmin - center + 0.5) * ss);
    int* k = kk + (size_t)xx * ksize;
    int x = 0;
    for (; x < xmax; ++x) {
      double w = f((x + xmin - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
      k[x] = w < 0 ? (int)(-0.5 + w * (1 << RS_PRECISION_BITS)) : (int)(0.5 + w * (1 << RS_PRECISION_BITS));
    }
    for (; x < ksize; ++x) k[x] = 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return 0;
}

int td_image_resize_u8_launch(const unsigned char* src, int in_h, int in_w, int in_c, unsigned char* dst, int out_h, int out_w, int out_c, const int* h_bounds,
                              const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, unsigned char* tmp, hipStream_t stream) {
  TD_CHECK_ARG(in_h > 0 && in_w > 0, "td_image_resize_u8: source size in_h=%d, in_w=%d must be positive", in_h, in_w);
  TD_CHECK_ARG(out_h > 0 && out_w > 0, "td_image_resize_u8: destination size out_h=%d, out_w=%d must be positive", out_h, out_w);
  TD_CHECK_ARG((in_c == 3 && out_c == 3) || (in_c == 1 && out_c == 1) || (in_c == 1 && out_c == 3) || (in_c == 4 && out_c == 3),
               "td_image_resize_u8: channels in_c=%d -> out_c=%d; 3 -> 3 (RGB), 1 -> 1 (L), 1 -> 3 (L replicated) and 4 -> 3 (RGBA, alpha dropped) are built", in_c, out_c);
  TD_CHECK_ARG(src && dst, "td_image_resize_u8: src or dst is null");
  const bool horiz = out_w != in_w, vert = out_h != in_h;
  TD_CHECK_ARG(!horiz || (h_bounds && h_kk && h_ksize > 0), "td_image_resize_u8: in_w=%d -> out_w=%d needs the horizontal table (bounds, kk, ksize=%d)", in_w, out_w, h_ksize);
  TD_CHECK_ARG(!vert || (v_bounds && v_kk && v_ksize > 0), "td_image_resize_u8: in_h=%d -> out_h=%d needs the vertical table (bounds, kk, ksize=%d)", in_h, out_h, v_ksize);
  TD_CHECK_ARG(!(horiz && vert) || tmp, "td_image_resize_u8: tmp is null; both axes change, so in_h * out_w * out_c = %lld bytes lie between the passes",
               (long long)in_h * out_w * out_c);
  // every index in the kernels is a 32-bit int over one of these three counts
  const long long n_src = (long long)in_h * in_w * in_c, n_mid = (long long)in_h * out_w * out_c, n_dst = (long long)out_h * out_w * out_c;
  TD_GRID_1D_I32(nblk_src, n_src, RS_THREADS, "td_image_resize_u8(source)");
  TD_GRID_1D_I32(nblk_mid, n_mid, RS_THREADS, "td_image_resize_u8(horizontal pass)");
  TD_GRID_1D_I32(nblk_dst, n_dst, RS_THREADS, "td_image_resize_u8(destination)");
  (void)nblk_src; (void)nblk_mid;
  if (!horiz && !vert) {
    hipLaunchKernelGGL(td_resize_copy_kernel, dim3(nblk_dst), dim3(RS_THREADS), 0, stream, src, in_c, dst, out_c, (int)n_dst);
    TD_CHECK_LAUNCH();
    return 0;
  }
  // the passes launch whole rows: rows x ceil(row bytes / block) workgroups, at most one block per row more than the counts above
  const int chunks = (int)(((long long)out_w * out_c + RS_THREADS - 1) / RS_THREADS);
  TD_GRID_1D(nblk_h, (long long)in_h * chunks * RS_THREADS, RS_THREADS, "td_image_resize_u8(horizontal pass, whole rows)");
  TD_GRID_1D(nblk_v, (long long)out_h * chunks * RS_THREADS, RS_THREADS, "td_image_resize_u8(vertical pass, whole rows)");
  const unsigned char* vsrc = src;
  int v_in_c = in_c;
  if (horiz) {
    unsigned char* hdst = vert ? tmp : dst;
    hipLaunchKernelGGL(td_resize_h_kernel, dim3(nblk_h), dim3(RS_THREADS), 0, stream, src, in_w, in_c, hdst, out_w, out_c, h_bounds, h_kk, h_ksize, chunks);
    TD_CHECK_LAUNCH();
    vsrc = hdst;
    v_in_c = out_c;
  }
  if (vert) {
    hipLaunchKernelGGL(td_resize_v_kernel, dim3(nblk_v), dim3(RS_THREADS), 0, stream, vsrc, in_h, out_w, v_in_c, dst, out_c, v_bounds, v_kk, v_ksize, chunks);
    TD_CHECK_LAUNCH();
  }
  return 0;
}

int td_image_lut_chw_f32_launch(const unsigned char* img, int H, int W, int C, const float* lut, float* out, hipStream_t stream) {
  TD_CHECK_ARG(H > 0 && W > 0 && C > 0 && C <= 4, "td_image_lut_chw_f32: image H=%d, W=%d, C=%d must be positive with at most 4 channels", H, W, C);
  TD_CHECK_ARG(img && lut && out, "td_image_lut_chw_f32: img, lut or out is null");
  const long long n = (long long)H * W * C;
  TD_GRID_1D_I32(nblk, n, RS_THREADS, "td_image_lut_chw_f32");
  hipLaunchKernelGGL(td_image_lut_chw_kernel, dim3(nblk), dim3(RS_THREADS), 0, stream, img, H * W, C, lut, out, (int)n);
  TD_CHECK_LAUNCH();
  return 0;
}
