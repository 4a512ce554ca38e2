// FLUX VAE encoder engine (AutoencoderKL.encode) and the two row kernels at its boundaries, all on the HIP kernels.
//
// Replaces, inside [ext] diffusers 0.31.0 FluxImg2ImgPipeline.__call__: `image_processor.preprocess` (uint8 / [0,1] image ->
// 2x - 1 in bf16), `vae.encode` ([ext] autoencoder_kl.py / vae.py Encoder with FLUX.1's vae/config.json: conv_in, 4
// DownEncoderBlock2D (ResnetBlock2D x layers_per_block + Downsample2D(use_conv, padding=0) on every block but the last),
// UNetMidBlock2D (ResnetBlock2D, single-head Attention, ResnetBlock2D), GroupNorm + SiLU, conv_out to 2 x latent_channels
// (double_z, no quant_conv)), `latent_dist.sample()` / `.mode()`, `_encode_vae_image`'s shift / scale, the scheduler's
// `scale_noise` and `_pack_latents`.
//
// Layout and kernels are the decoder's (vae_engine.hip): NHWC rows, every 3x3 conv an implicit GEMM on the MFMA GEMM kernel;
// Downsample2D's pad (0,1,0,1) + stride-2 conv is the GEMM's stride-2 conv form (conv_s2); the mid-block attention is the
// decoder's chunked fp32-score path (vae_common.h).
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "vae_common.h"
#include "../../include/thinkdiff_hip.h"

using namespace tdvae;

struct td_vae_enc {
  TdVaeConfig cfg;
  int nb = 0, cmid = 0, in_pad = 0, mom_c = 0, max_pixels = 0;
  bf16_t* arena = nullptr;
  std::vector<VSlot> slots;
  std::unordered_map<std::string, int> index;
  bf16_t *cin_w, *cin_b, *nout_w, *nout_b, *cout_w, *cout_b;
  std::vector<std::vector<Resnet>> down;
  std::vector<bf16_t*> ds_w, ds_b;
  Resnet mid[2];
  MidAttn attn;
  // workspace
  char* ws = nullptr;
  bf16_t *X, *T1, *T2, *T3, *Q, *K, *VT, *P;
  float *S, *gn;
  int chunk_rows = 0;
};

namespace {

// ---- VaeImageProcessor.preprocess + .to(bf16): image -> NHWC [H*W, Cpad] bf16, channels >= 3 zero --------------------------------
// uint8 HWC: x = float32(u8) / 255 (pil_to_numpy), 2x - 1 (normalize), RNE to bf16; float32 CHW in [0,1]: 2x - 1, RNE to bf16.
// Every step is one IEEE fp32 operation (explicit _rn intrinsics: no contraction into an fma), as numpy / torch compute it.
// One thread per (pixel, 8-channel chunk): 16-byte stores.
// MASKED (FLUX.1 Fill, [ext] diffusers >= 0.32 pipeline_flux_fill.py `masked_image = image * (1 - mask)` on the fp32 preprocessed image, then
// `.to(bf16)`): the value is multiplied by 1 - m in fp32 before the rounding, m = the binarized mask pixel (u8 >= 128, f32 >= 0.5; [H, W] at
// full resolution).  With m in {0, 1} that is the unmasked value or a zero carrying its sign.
template <bool MASKED>
__global__ void td_vae_image_in_kernel(const void* src, int fmt, int H, int W, bf16_t* out, int Cpad, const void* mask, int mfmt) {
  const int chunks = Cpad >> 3;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * W * chunks) return;
  const int pix = idx / chunks, ch = idx - pix * chunks;
  u32x4_t o = {0u, 0u, 0u, 0u};
  if (ch == 0) {
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = fmt == TD_IMAGE_U8_HWC ? __fdiv_rn((float)((const unsigned char*)src)[(size_t)pix * 3 + c], 255.0f)
                                             : ((const float*)src)[(size_t)c * H * W + pix];
      v[c] = __fsub_rn(__fmul_rn(2.0f, x), 1.0f);
    }
    if (MASKED) {
      const bool on = mfmt == TD_INPAINT_MASK_U8_HW ? ((const unsigned char*)mask)[pix] >= 128 : ((const float*)mask)[pix] >= 0.5f;
      const float keep = __fsub_rn(1.0f, on ? 1.0f : 0.0f);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = __fmul_rn(v[c], keep);
    }
    o[0] = pack_bf2(v[0], v[1]);
    o[1] = pack_bf2(v[2], 0.f);
  }
  *(u32x4_t*)(out + (size_t)pix * Cpad + ch * 8) = o;
}

// mask == NULL: the plain image; else the masked image (mfmt = TD_INPAINT_MASK_*)
int image_in_launch(const void* src, int fmt, int H, int W, bf16_t* out, int Cpad, hipStream_t s, const void* mask = nullptr, int mfmt = 0) {
  TD_CHECK_ARG(src && out && H > 0 && W > 0 && Cpad >= 8 && Cpad % 8 == 0, "td_vae_image_to_nhwc: bad arguments");
  TD_CHECK_ARG(!mask || mfmt == TD_INPAINT_MASK_U8_HW || mfmt == TD_INPAINT_MASK_F32_HW, "td_vae_image_to_nhwc: unknown mask format %d", mfmt);
  TD_CHECK_ARG(fmt == TD_IMAGE_U8_HWC || fmt == TD_IMAGE_F32_CHW, "td_vae_image_to_nhwc: unknown image format %d", fmt);
  TD_CHECK_ARG(((uintptr_t)out) % 16 == 0, "td_vae_image_to_nhwc: out must be 16-byte aligned");
  TD_GRID_1D_I32(nblk, (long long)H * W * (Cpad / 8), 256, "td_vae_image_to_nhwc");
  if (mask) hipLaunchKernelGGL(td_vae_image_in_kernel<true>, dim3(nblk), dim3(256), 0, s, src, fmt, H, W, out, Cpad, mask, mfmt);
  else hipLaunchKernelGGL(td_vae_image_in_kernel<false>, dim3(nblk), dim3(256), 0, s, src, fmt, H, W, out, Cpad, (const void*)nullptr, 0);
  TD_CHECK_LAUNCH();
  return 0;
}

// ---- moments [h*w, 2C] (mean | logvar) -> packed FLUX latents [(h/2)(w/2), 4C] ---------------------------------------------------
// The rounding points of the bf16 torch statements (one op = fp32 arithmetic on bf16 values, result rounded to bf16):
//   DiagonalGaussianDistribution: logvar = clamp(logvar, -30, 20); std = exp(0.5 * logvar); z = mean + std * eps  (eps NULL: z = mean)
//   _encode_vae_image:            z = (z - shift) * scaling   (torch: the subtracted python scalar is cast to bf16, the factor stays fp32)
//   scale_noise:                  x = sigma * noise + (1 - sigma) * z   with sigma = bf16(sigma)            (noise NULL: x = z)
//   _pack_latents:                row (y/2)(w/2) + x/2, column 4c + 2(y&1) + (x&1)
// eps / noise are NCHW [C, h, w] bf16 (what torch.randn(..., dtype=bf16) draws for one image).
// latent_value: column `col` of packed token `tok` (shared by td_vae_latents_kernel and td_flux_fill_condition_kernel, as euler8 is shared by the
// two step kernels); the result is a bf16 value held in fp32.
__device__ __forceinline__ float latent_value(const bf16_t* mom, const bf16_t* eps, const bf16_t* noise, float sigma, float scaling, float shift,
                                              int C, int h, int w, int tok, int col) {
  const int c = col >> 2, y = (tok / (w >> 1)) * 2 + ((col >> 1) & 1), x = (tok % (w >> 1)) * 2 + (col & 1);
  const int pix = y * w + x;
  float z = bf2f(mom[(size_t)pix * 2 * C + c]);
  if (eps) {
    const float lv = fminf(fmaxf(bf2f(mom[(size_t)pix * 2 * C + C + c]), -30.f), 20.f);
    const float sd = rbf(expf(rbf(__fmul_rn(0.5f, lv))));
    z = rbf(__fadd_rn(z, rbf(__fmul_rn(sd, bf2f(eps[(size_t)c * h * w + pix])))));
  }
  z = rbf(__fmul_rn(rbf(__fsub_rn(z, rbf(shift))), scaling));
  if (noise) {
    const float s = rbf(sigma);
    z = rbf(__fadd_rn(rbf(__fmul_rn(s, bf2f(noise[(size_t)c * h * w + pix]))), rbf(__fmul_rn(rbf(__fsub_rn(1.0f, s)), z))));
  }
  return z;
}

__global__ void td_vae_latents_kernel(const bf16_t* mom, const bf16_t* eps, const bf16_t* noise, float sigma, float scaling, float shift,
                                      int C, int h, int w, bf16_t* out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= h * w * C) return;
  out[idx] = f2bf(latent_value(mom, eps, noise, sigma, scaling, shift, C, h, w, idx / (4 * C), idx % (4 * C)));
}

// ---- FLUX.1 Fill's channel condition of one image: [S, 4C + 256] = packed masked-image latents | unshuffled mask ------------------
// [ext] diffusers >= 0.32 pipeline_flux_fill.py prepare_mask_latents:
//   masked_image_latents = _pack_latents((vae.encode(masked_image).latent_dist.sample(generator) - shift) * scaling)
//   mask = mask[:, 0].view(B, h, 8, w, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, h, w);  mask = _pack_latents(mask)
//   masked_image_latents = torch.cat((masked_image_latents, mask), dim=-1)
// The first 4C columns are latent_value with noise = NULL.  Mask column (py*8 + px)*4 + dy*2 + dx of token (Y, X) is the binarized mask
// pixel (8(2Y + dy) + py, 8(2X + dx) + px): every pixel of the 16 x 16 patch of a token lands in exactly one of its 256 columns.
// One lane per 8 output columns (16-byte stores): latent chunk j = channels 2j, 2j+1; mask chunk k = (py, px) in {(k >> 2, 2 (k & 3)), +1 in px},
// whose two mask pixels per (dy, dx) are neighbours in the row.
__global__ void td_flux_fill_condition_kernel(const bf16_t* mom, const bf16_t* eps, const void* mask, int mfmt, int H, int W, float scaling,
                                              float shift, int C, bf16_t* out) {
  const int h = H >> 3, w = W >> 3, lat_chunks = C >> 1, chunks = lat_chunks + 32;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (h >> 1) * (w >> 1) * chunks) return;
  const int tok = idx / chunks, ch = idx - tok * chunks;
  float v[8];
  if (ch < lat_chunks) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = latent_value(mom, eps, nullptr, 0.f, scaling, shift, C, h, w, tok, ch * 8 + i);
  } else {
    const int k = ch - lat_chunks, py = k >> 2, px = 2 * (k & 3);
    const int Y = tok / (w >> 1), X = tok - Y * (w >> 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {      // i = (px & 1) * 4 + dy * 2 + dx
      const size_t pix = (size_t)(8 * (2 * Y + ((i >> 1) & 1)) + py) * W + 8 * (2 * X + (i & 1)) + px + (i >> 2);
      const bool on = mfmt == TD_INPAINT_MASK_U8_HW ? ((const unsigned char*)mask)[pix] >= 128 : ((const float*)mask)[pix] >= 0.5f;
      v[i] = on ? 1.0f : 0.0f;
    }
  }
  *(u32x4_t*)(out + (size_t)tok * (4 * C + 256) + ch * 8) =
      u32x4_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
}

int conv3_s2(hipStream_t s, const bf16_t* x, const bf16_t* w, const bf16_t* b, bf16_t* y, int Hout, int Wout, int cin, int cout) {
  TdGemmParams p;
  p.A = x; p.lda = cin; p.W = w; p.bias = b; p.C = y; p.ldc = cout;
  p.M = Hout * Wout; p.N = cout; p.K = 9 * cin; p.conv_H = Hout; p.conv_W = Wout; p.conv_Cin = cin; p.conv_s2 = 1;
  return td_gemm_launch(p, s);
}

}  // namespace

extern "C" {

int td_conv3x3_s2_nhwc_bf16(const void* x, const void* w, const void* bias, void* y, int Hin, int Win, int Cin, int Cout, void* stream) {
  TD_CHECK_ARG(Hin > 0 && Win > 0 && Hin % 2 == 0 && Win % 2 == 0, "td_conv3x3_s2_nhwc_bf16: input %dx%d must be even", Hin, Win);
  return conv3_s2((hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)bias, (bf16_t*)y, Hin / 2, Win / 2, Cin, Cout);
}

int td_vae_image_to_nhwc_bf16(const void* image, int image_format, int H, int W, void* out, int Cpad, void* stream) {
  return image_in_launch(image, image_format, H, W, (bf16_t*)out, Cpad, (hipStream_t)stream);
}

int td_vae_image_to_nhwc_masked_bf16(const void* image, int image_format, const void* mask, int mask_format, int H, int W, void* out, int Cpad,
                                     void* stream) {
  TD_CHECK_ARG(mask, "td_vae_image_to_nhwc_masked: null mask");
  return image_in_launch(image, image_format, H, W, (bf16_t*)out, Cpad, (hipStream_t)stream, mask, mask_format);
}

int td_flux_fill_condition(const void* moments, const void* eps, const void* mask, int mask_format, int H, int W, float scaling_factor,
                           float shift_factor, int C, void* cond_out, void* stream) {
  TD_CHECK_ARG(moments && mask && cond_out, "td_flux_fill_condition: null argument (moments, mask and cond_out are required)");
  TD_CHECK_ARG(mask_format == TD_INPAINT_MASK_U8_HW || mask_format == TD_INPAINT_MASK_F32_HW, "td_flux_fill_condition: unknown mask format %d", mask_format);
  TD_CHECK_ARG(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "td_flux_fill_condition: H=%d, W=%d must be positive multiples of 16", H, W);
  TD_CHECK_ARG(C > 0 && C % 2 == 0, "td_flux_fill_condition: C=%d must be a positive multiple of 2 (4C columns in 8-column chunks)", C);
  TD_CHECK_ARG(((uintptr_t)cond_out) % 16 == 0, "td_flux_fill_condition: cond_out must be 16-byte aligned");
  TD_GRID_1D_I32(nblk, (long long)(H / 16) * (W / 16) * (C / 2 + 32), 256, "td_flux_fill_condition");
  hipLaunchKernelGGL(td_flux_fill_condition_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)moments, (const bf16_t*)eps,
                     mask, mask_format, H, W, scaling_factor, shift_factor, C, (bf16_t*)cond_out);
  TD_CHECK_LAUNCH();
  return TD_OK;
}

int td_vae_latents_from_moments(const void* moments, const void* eps, const void* noise, float sigma, float scaling_factor,
                                float shift_factor, int C, int h, int w, void* packed_out, void* stream) {
  TD_CHECK_ARG(moments && packed_out, "td_vae_latents_from_moments: null argument");
  TD_CHECK_ARG(C > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, "td_vae_latents_from_moments: C=%d, h=%d, w=%d (h, w must be even)", C, h, w);
  TD_GRID_1D_I32(nblk, (long long)h * w * C, 256, "td_vae_latents_from_moments");
  hipLaunchKernelGGL(td_vae_latents_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)moments, (const bf16_t*)eps,
                     (const bf16_t*)noise, sigma, scaling_factor, shift_factor, C, h, w, (bf16_t*)packed_out);
  TD_CHECK_LAUNCH();
  return TD_OK;
}

int td_vae_enc_create(const TdVaeConfig* cfg, int max_image_h, int max_image_w, td_vae_enc** out) {
  TD_CHECK_ARG(cfg && out && max_image_h > 0 && max_image_w > 0, "td_vae_enc_create: bad arguments");
  TD_CHECK_ARG(cfg->num_blocks >= 1 && cfg->num_blocks <= 4, "td_vae_enc_create: 1..4 blocks supported");
  TD_CHECK_ARG(cfg->out_channels == 3, "td_vae_enc_create: the image-in kernel feeds 3 channels (out_channels = %d)", cfg->out_channels);
  TD_CHECK_ARG(cfg->latent_channels > 0 && (2 * cfg->latent_channels) % 8 == 0, "td_vae_enc_create: 2 x latent_channels must be a multiple of 8");
  for (int i = 0; i < cfg->num_blocks; ++i)
    TD_CHECK_ARG(cfg->block_out_channels[i] % 64 == 0 && cfg->block_out_channels[i] % cfg->norm_groups == 0,
                 "td_vae_enc_create: block_out_channels must be multiples of 64 and of norm_groups");
  td_vae_enc* f = new td_vae_enc();
  f->cfg = *cfg;
  const int nb = f->nb = cfg->num_blocks;
  const int cmid = f->cmid = cfg->block_out_channels[nb - 1];
  const int c0 = cfg->block_out_channels[0];
  f->in_pad = pad64(cfg->out_channels);
  f->mom_c = 2 * cfg->latent_channels;
  f->max_pixels = max_image_h * max_image_w;

  Plan pl;
  pl.take(&f->cin_w, (int64_t)c0 * 9 * f->in_pad); pl.take(&f->cin_b, c0);
  f->down.resize(nb); f->ds_w.assign(nb, nullptr); f->ds_b.assign(nb, nullptr);
  int prev = c0;
  for (int b = 0; b < nb; ++b) {
    const int co = cfg->block_out_channels[b];
    f->down[b].resize(cfg->layers_per_block);
    for (int r = 0; r < cfg->layers_per_block; ++r) plan_resnet(pl, f->down[b][r], r == 0 ? prev : co, co);
    if (b != nb - 1) { pl.take(&f->ds_w[b], (int64_t)co * 9 * co); pl.take(&f->ds_b[b], co); }
    prev = co;
  }
  plan_resnet(pl, f->mid[0], cmid, cmid);
  plan_attn(pl, f->attn, cmid);
  plan_resnet(pl, f->mid[1], cmid, cmid);
  pl.take(&f->nout_w, cmid); pl.take(&f->nout_b, cmid);
  pl.take(&f->cout_w, (int64_t)f->mom_c * 9 * cmid); pl.take(&f->cout_b, f->mom_c);
  hipError_t e = hipMalloc((void**)&f->arena, (size_t)pl.off * 2);
  if (e != hipSuccess) { td_set_error("td_vae_enc_create: weight hipMalloc failed: %s", hipGetErrorString(e)); delete f; return TD_ERR_HIP; }
  (void)hipMemset(f->arena, 0, (size_t)pl.off * 2);   // padded input channels of conv_in must be zero
  (void)hipDeviceSynchronize();   // the handle may be used from any stream next; a null-stream memset is not ordered with non-blocking streams
  for (auto& fx : pl.fix) *fx.first = f->arena + fx.second;

  // diffusers state-dict names
  v_add(f, "encoder.conv_in.weight", f->cin_w, (int64_t)c0 * cfg->out_channels * 9, 1, c0, cfg->out_channels, c0, f->in_pad);
  v_add(f, "encoder.conv_in.bias", f->cin_b, c0);
  for (int b = 0; b < nb; ++b) {
    const std::string db = "encoder.down_blocks." + std::to_string(b) + ".";
    for (int r = 0; r < cfg->layers_per_block; ++r) name_resnet(f, db + "resnets." + std::to_string(r) + ".", f->down[b][r]);
    if (f->ds_w[b]) {
      const int co = cfg->block_out_channels[b];
      v_add(f, db + "downsamplers.0.conv.weight", f->ds_w[b], (int64_t)co * co * 9, 1, co, co, co, co);
      v_add(f, db + "downsamplers.0.conv.bias", f->ds_b[b], co);
    }
  }
  name_resnet(f, "encoder.mid_block.resnets.0.", f->mid[0]);
  name_attn(f, "encoder.mid_block.attentions.0.", f->attn, cmid);
  name_resnet(f, "encoder.mid_block.resnets.1.", f->mid[1]);
  v_add(f, "encoder.conv_norm_out.weight", f->nout_w, cmid); v_add(f, "encoder.conv_norm_out.bias", f->nout_b, cmid);
  v_add(f, "encoder.conv_out.weight", f->cout_w, (int64_t)f->mom_c * cmid * 9, 1, f->mom_c, cmid, f->mom_c, cmid);
  v_add(f, "encoder.conv_out.bias", f->cout_b, f->mom_c);

  // workspace: largest image buffers along the encode path (X / T1 also hold the padded input image and a downsampler's output)
  int64_t px = f->max_pixels, maxX = px * std::max(f->in_pad, c0), maxT2 = px * c0;
  prev = c0;
  for (int b = 0; b < nb; ++b) {
    const int co = cfg->block_out_channels[b];
    maxX = std::max(maxX, px * std::max(prev, co));
    maxT2 = std::max(maxT2, px * co);
    if (b != nb - 1) px /= 4;
    prev = co;
  }
  const int64_t pm = px;   // mid-block pixels at capacity
  const int64_t pk = (pm + 63) & ~int64_t(63);   // ... and its key axis, padded to the GEMM's k-tile (mid_attention)
  maxX = std::max(maxX, pk * cmid);              // T1 carries the pad rows of gn(x)
  f->chunk_rows = (int)std::min<int64_t>(2048, pm);
  struct Req { void** p; int64_t bytes; };
  std::vector<Req> reqs = {
      {(void**)&f->X, maxX * 2}, {(void**)&f->T1, maxX * 2}, {(void**)&f->T2, maxT2 * 2}, {(void**)&f->T3, maxT2 * 2},
      {(void**)&f->Q, pm * cmid * 2}, {(void**)&f->K, pk * cmid * 2}, {(void**)&f->VT, pk * cmid * 2},
      {(void**)&f->S, (int64_t)f->chunk_rows * pk * 4}, {(void**)&f->P, (int64_t)f->chunk_rows * pk * 2},
      {(void**)&f->gn, (int64_t)(1024 * 64 * 2 + 256) * 4},
  };
  int64_t total = 0;
  for (auto& r : reqs) total += (r.bytes + 255) & ~int64_t(255);
  e = hipMalloc((void**)&f->ws, (size_t)total);
  if (e != hipSuccess) {
    td_set_error("td_vae_enc_create: hipMalloc of %.2f GiB workspace failed: %s", total / double(1 << 30), hipGetErrorString(e));
    (void)hipFree(f->arena); delete f; return TD_ERR_HIP;
  }
  int64_t o = 0;
  for (auto& r : reqs) { *r.p = f->ws + o; o += (r.bytes + 255) & ~int64_t(255); }
  *out = f;
  return TD_OK;
}

void td_vae_enc_destroy(td_vae_enc* f) {
  if (!f) return;
  (void)hipFree(f->arena);
  (void)hipFree(f->ws);
  delete f;
}

int td_vae_enc_num_params(const td_vae_enc* f) { return f ? (int)f->slots.size() : 0; }

int td_vae_enc_param_info(const td_vae_enc* f, int idx, char* name_buf, int buf_len, int64_t* count) {
  return param_info(f, "td_vae_enc_param_info", idx, name_buf, buf_len, count);
}

int td_vae_enc_load_param(td_vae_enc* f, const char* name, const void* src, int64_t count, void* stream) {
  return load_param(f, "td_vae_enc_load_param", name, src, count, stream);
}

int td_vae_enc_init_random(td_vae_enc* f, uint64_t seed, float std, void* stream) {
  return init_random(f, "td_vae_enc_init_random", seed, std, stream);
}

int td_vae_enc_output_shape(const td_vae_enc* f, int H, int W, int* h, int* w, int* moment_channels) {
  TD_CHECK_ARG(f && H > 0 && W > 0, "td_vae_enc_output_shape: null context or empty image");
  if (h) *h = H >> (f->nb - 1);
  if (w) *w = W >> (f->nb - 1);
  if (moment_channels) *moment_channels = f->mom_c;
  return TD_OK;
}

static int vae_encode(td_vae_enc* f, const void* image, int image_format, const void* mask, int mask_format, int H, int W, void* moments_nhwc,
                      void* stream);

int td_vae_encode(td_vae_enc* f, const void* image, int image_format, int H, int W, void* moments_nhwc, void* stream) {
  return vae_encode(f, image, image_format, nullptr, 0, H, W, moments_nhwc, stream);
}

int td_vae_encode_masked(td_vae_enc* f, const void* image, int image_format, const void* mask, int mask_format, int H, int W,
                         void* moments_nhwc, void* stream) {
  TD_CHECK_ARG(mask, "td_vae_encode_masked: null mask");
  TD_CHECK_ARG(mask_format == TD_INPAINT_MASK_U8_HW || mask_format == TD_INPAINT_MASK_F32_HW, "td_vae_encode_masked: unknown mask format %d", mask_format);
  return vae_encode(f, image, image_format, mask, mask_format, H, W, moments_nhwc, stream);
}

// mask == NULL: td_vae_encode; else td_vae_encode_masked (only the image-in stage differs)
static int vae_encode(td_vae_enc* f, const void* image, int image_format, const void* mask, int mask_format, int H, int W, void* moments_nhwc,
                      void* stream) {
  TD_CHECK_ARG(f && image && moments_nhwc, "td_vae_encode: null argument");
  TD_CHECK_ARG(image_format == TD_IMAGE_U8_HWC || image_format == TD_IMAGE_F32_CHW, "td_vae_encode: unknown image format %d", image_format);
  TD_CHECK_ARG(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "td_vae_encode: image %dx%d: height and width must be positive multiples of 16", H, W);
  TD_CHECK_ARG((long long)H * W <= f->max_pixels, "td_vae_encode: image %dx%d exceeds the %d-pixel capacity given at create", H, W, f->max_pixels);
  const int nb = f->nb, cmid = f->cmid;
  TD_CHECK_ARG(((uintptr_t)moments_nhwc) % 16 == 0, "td_vae_encode: moments must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;

  TDV_TRY(image_in_launch(image, image_format, H, W, f->T1, f->in_pad, s, mask, mask_format));
  TDV_TRY(conv3(s, f->T1, f->cin_w, f->cin_b, nullptr, f->X, H, W, f->in_pad, f->cfg.block_out_channels[0], 0));
  // ---- down blocks ----------------------------------------------------------------------------------------
  for (int b = 0; b < nb; ++b) {
    for (auto& r : f->down[b]) TDV_TRY(resnet(f, s, r, H, W));
    if (f->ds_w[b]) {   // Downsample2D: pad (0,1,0,1) + 3x3 stride 2, fused; output replaces X via T1
      const int co = f->cfg.block_out_channels[b];
      H /= 2; W /= 2;
      TDV_TRY(conv3_s2(s, f->X, f->ds_w[b], f->ds_b[b], f->T1, H, W, co, co));
      std::swap(f->X, f->T1);
    }
  }
  // ---- mid block ------------------------------------------------------------------------------------------
  TDV_TRY(resnet(f, s, f->mid[0], H, W));
  TDV_TRY(mid_attention(f, s, f->attn, H * W, cmid));
  TDV_TRY(resnet(f, s, f->mid[1], H, W));
  TDV_TRY(gn(f, s, f->X, f->T1, H * W, cmid, f->nout_w, f->nout_b, 1));
  TDV_TRY(conv3(s, f->T1, f->cout_w, f->cout_b, nullptr, (bf16_t*)moments_nhwc, H, W, cmid, f->mom_c, 0));
  return TD_OK;
}

}  // extern "C"
