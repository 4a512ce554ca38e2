// FLUX VAE decoder engine (AutoencoderKL.decode): packed latents -> uint8 image, all on the HIP kernels.
//
// Replaces, inside the reference drivers' `diffusion_pipe(...)` call
// (scripts/test/test_blip_vision_t5_decoder_flux_text.py:234-242), the tail of [ext] diffusers 0.31.0
// FluxPipeline.__call__: `_unpack_latents`, `latents / scaling_factor + shift_factor`,
// `vae.decode` ([ext] autoencoder_kl.py / vae.py Decoder: conv_in, UNetMidBlock2D (ResnetBlock2D, single-head
// Attention, ResnetBlock2D), 4 UpDecoderBlock2D (3 ResnetBlock2D + Upsample2D), GroupNorm, SiLU, conv_out) and
// `image_processor.postprocess` (denormalise, uint8).
//
// Layout: images are NHWC ([pixels, channels] rows), so every 3x3 conv is an implicit GEMM on the MFMA GEMM
// kernel (no im2col buffer, zero padding and the nearest 2x upsample folded into the A-operand addressing),
// 1x1 convs and the attention projections are plain GEMMs, GroupNorm+SiLU is a 3-launch row kernel.
// The mid-block attention has ONE head of width 512: scores are produced in fp32 row chunks by the GEMM
// (fp32 output), softmaxed by a row kernel and multiplied with V^T by the GEMM again; to_v's bias is added
// after the product (softmax rows sum to 1).
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include <algorithm>
#include <cmath>

#include "vae_common.h"
#include "../../include/thinkdiff_hip.h"

using namespace tdvae;

struct td_vae {
  TdVaeConfig cfg;
  int nb = 0, cmid = 0, lat_pad = 0, out_pad = 0, max_lat_pixels = 0;
  bf16_t* arena = nullptr;
  int64_t arena_elems = 0;
  std::vector<VSlot> slots;
  std::unordered_map<std::string, int> index;
  bf16_t *cin_w, *cin_b, *nout_w, *nout_b, *cout_w, *cout_b;
  Resnet mid[2];
  MidAttn attn;
  std::vector<std::vector<Resnet>> up;
  std::vector<bf16_t*> ups_w, ups_b;
  // workspace
  char* ws = nullptr;
  bf16_t *X, *T1, *T2, *T3, *Q, *K, *VT, *P;
  float *S, *gn;
  int chunk_rows = 0;
};

extern "C" {

int td_vae_create(const TdVaeConfig* cfg, int max_latent_h, int max_latent_w, td_vae** out) {
  TD_CHECK_ARG(cfg && out && max_latent_h > 0 && max_latent_w > 0, "td_vae_create: bad arguments");
  TD_CHECK_ARG(cfg->num_blocks >= 1 && cfg->num_blocks <= 4, "td_vae_create: 1..4 blocks supported");
  for (int i = 0; i < cfg->num_blocks; ++i)
    TD_CHECK_ARG(cfg->block_out_channels[i] % 64 == 0 && cfg->block_out_channels[i] % cfg->norm_groups == 0,
                 "td_vae_create: block_out_channels must be multiples of 64 and of norm_groups");
  td_vae* f = new td_vae();
  f->cfg = *cfg;
  const int nb = f->nb = cfg->num_blocks;
  const int cmid = f->cmid = cfg->block_out_channels[nb - 1];
  f->lat_pad = pad64(cfg->latent_channels);
  f->out_pad = pad8(cfg->out_channels);
  f->max_lat_pixels = max_latent_h * max_latent_w;

  Plan pl;
  pl.take(&f->cin_w, (int64_t)cmid * 9 * f->lat_pad); pl.take(&f->cin_b, cmid);
  plan_resnet(pl, f->mid[0], cmid, cmid);
  plan_resnet(pl, f->mid[1], cmid, cmid);
  plan_attn(pl, f->attn, cmid);
  f->up.resize(nb); f->ups_w.assign(nb, nullptr); f->ups_b.assign(nb, nullptr);
  int prev = cmid;
  for (int b = 0; b < nb; ++b) {   // reversed block_out_channels
    const int co = cfg->block_out_channels[nb - 1 - b];
    f->up[b].resize(cfg->layers_per_block + 1);
    for (int r = 0; r <= cfg->layers_per_block; ++r) plan_resnet(pl, f->up[b][r], r == 0 ? prev : co, co);
    if (b != nb - 1) { pl.take(&f->ups_w[b], (int64_t)co * 9 * co); pl.take(&f->ups_b[b], co); }
    prev = co;
  }
  const int clast = cfg->block_out_channels[0];
  pl.take(&f->nout_w, clast); pl.take(&f->nout_b, clast);
  pl.take(&f->cout_w, (int64_t)f->out_pad * 9 * clast); pl.take(&f->cout_b, f->out_pad);
  f->arena_elems = pl.off;
  hipError_t e = hipMalloc((void**)&f->arena, (size_t)pl.off * 2);
  if (e != hipSuccess) { td_set_error("td_vae_create: weight hipMalloc failed: %s", hipGetErrorString(e)); delete f; return TD_ERR_HIP; }
  (void)hipMemset(f->arena, 0, (size_t)pl.off * 2);   // padded weight rows / channels must be zero
  (void)hipDeviceSynchronize();   // the handle may be used from any stream next; a null-stream memset is not ordered with non-blocking streams
  for (auto& fx : pl.fix) *fx.first = f->arena + fx.second;

  // diffusers state-dict names
  v_add(f, "decoder.conv_in.weight", f->cin_w, (int64_t)cmid * cfg->latent_channels * 9, 1, cmid, cfg->latent_channels, cmid, f->lat_pad);
  v_add(f, "decoder.conv_in.bias", f->cin_b, cmid);
  name_resnet(f, "decoder.mid_block.resnets.0.", f->mid[0]);
  name_resnet(f, "decoder.mid_block.resnets.1.", f->mid[1]);
  name_attn(f, "decoder.mid_block.attentions.0.", f->attn, cmid);
  for (int b = 0; b < nb; ++b) {
    const std::string ub = "decoder.up_blocks." + std::to_string(b) + ".";
    for (int r = 0; r <= cfg->layers_per_block; ++r) name_resnet(f, ub + "resnets." + std::to_string(r) + ".", f->up[b][r]);
    if (f->ups_w[b]) {
      const int co = f->up[b][0].cout;
      v_add(f, ub + "upsamplers.0.conv.weight", f->ups_w[b], (int64_t)co * co * 9, 1, co, co, co, co);
      v_add(f, ub + "upsamplers.0.conv.bias", f->ups_b[b], co);
    }
  }
  v_add(f, "decoder.conv_norm_out.weight", f->nout_w, clast); v_add(f, "decoder.conv_norm_out.bias", f->nout_b, clast);
  v_add(f, "decoder.conv_out.weight", f->cout_w, (int64_t)cfg->out_channels * clast * 9, 1, cfg->out_channels, clast, f->out_pad, clast);
  v_add(f, "decoder.conv_out.bias", f->cout_b, cfg->out_channels);

  // workspace: largest image buffers along the decode path
  int64_t maxX = (int64_t)f->max_lat_pixels * cmid, maxT2 = maxX, px = f->max_lat_pixels;
  prev = cmid;
  for (int b = 0; b < nb; ++b) {
    const int co = cfg->block_out_channels[nb - 1 - b];
    maxX = std::max(maxX, px * std::max(prev, co));
    maxT2 = std::max(maxT2, px * co);
    if (b != nb - 1) { px *= 4; maxX = std::max(maxX, px * co); }
    prev = co;
  }
  const int64_t pk = ((int64_t)f->max_lat_pixels + 63) & ~int64_t(63);   // the mid-block attention's key axis, padded to the GEMM's k-tile
  maxX = std::max(maxX, pk * cmid);                                      // T1 carries the pad rows of gn(x)
  f->chunk_rows = std::min(2048, f->max_lat_pixels);
  struct Req { void** p; int64_t bytes; };
  std::vector<Req> reqs = {
      {(void**)&f->X, maxX * 2}, {(void**)&f->T1, maxX * 2}, {(void**)&f->T2, maxT2 * 2}, {(void**)&f->T3, maxT2 * 2},
      {(void**)&f->Q, (int64_t)f->max_lat_pixels * cmid * 2}, {(void**)&f->K, pk * cmid * 2},
      {(void**)&f->VT, pk * cmid * 2},
      {(void**)&f->S, (int64_t)f->chunk_rows * pk * 4}, {(void**)&f->P, (int64_t)f->chunk_rows * pk * 2},
      {(void**)&f->gn, (int64_t)(1024 * 64 * 2 + 256) * 4},
  };
  int64_t total = 0;
  for (auto& r : reqs) total += (r.bytes + 255) & ~int64_t(255);
  e = hipMalloc((void**)&f->ws, (size_t)total);
  if (e != hipSuccess) {
    td_set_error("td_vae_create: hipMalloc of %.2f GiB workspace failed: %s", total / double(1 << 30), hipGetErrorString(e));
    (void)hipFree(f->arena); delete f; return TD_ERR_HIP;
  }
  int64_t o = 0;
  for (auto& r : reqs) { *r.p = f->ws + o; o += (r.bytes + 255) & ~int64_t(255); }
  *out = f;
  return TD_OK;
}

void td_vae_destroy(td_vae* f) {
  if (!f) return;
  (void)hipFree(f->arena);
  (void)hipFree(f->ws);
  delete f;
}

int td_vae_num_params(const td_vae* f) { return f ? (int)f->slots.size() : 0; }

int td_vae_param_info(const td_vae* f, int idx, char* name_buf, int buf_len, int64_t* count) {
  return param_info(f, "td_vae_param_info", idx, name_buf, buf_len, count);
}

int td_vae_load_param(td_vae* f, const char* name, const void* src, int64_t count, void* stream) {
  return load_param(f, "td_vae_load_param", name, src, count, stream);
}

int td_vae_init_random(td_vae* f, uint64_t seed, float std, void* stream) {
  return init_random(f, "td_vae_init_random", seed, std, stream);
}

// packed FLUX latents [ (h/2)(w/2), 4*latent_channels ] bf16 -> image.  h, w: latent height/width (image = 8h x 8w
// for the 4-block FLUX VAE).  image_u8: [H, W, 3] uint8 (may be NULL); image_chw: bf16 [3, H, W] = vae.decode output
// (may be NULL).  The z / scaling_factor + shift_factor step of the pipeline is applied first.
// Image size td_vae_decode writes for an h x w latent: one 2x upsampler behind every block but the last, and the packed latent's channel count.
int td_vae_output_shape(const td_vae* f, int h, int w, int* H, int* W, int* packed_channels) {
  TD_CHECK_ARG(f && h > 0 && w > 0, "td_vae_output_shape: null context or empty latent");
  if (H) *H = h << (f->nb - 1);
  if (W) *W = w << (f->nb - 1);
  if (packed_channels) *packed_channels = 4 * f->cfg.latent_channels;
  return TD_OK;
}

int td_vae_decode(td_vae* f, const void* packed_latents, int h, int w, float scaling_factor, float shift_factor,
                  void* image_u8, void* image_chw, void* stream) {
  TD_CHECK_ARG(f && packed_latents && (image_u8 || image_chw), "td_vae_decode: null argument");
  TD_CHECK_ARG(h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && h * w <= f->max_lat_pixels, "td_vae_decode: latent %dx%d exceeds the %d-pixel capacity", h, w, f->max_lat_pixels);
  hipStream_t s = (hipStream_t)stream;
  const int cmid = f->cmid, nb = f->nb;
  int H = h, W = w;
  const int P0 = H * W;

  TDV_TRY(td_latents_to_nhwc_launch((const bf16_t*)packed_latents, f->T1, f->cfg.latent_channels, h, w, f->lat_pad, scaling_factor, shift_factor, s));
  TDV_TRY(conv3(s, f->T1, f->cin_w, f->cin_b, nullptr, f->X, H, W, f->lat_pad, cmid, 0));

  // ---- mid block ------------------------------------------------------------------------------------------
  TDV_TRY(resnet(f, s, f->mid[0], H, W));
  TDV_TRY(mid_attention(f, s, f->attn, P0, cmid));
  TDV_TRY(resnet(f, s, f->mid[1], H, W));

  // ---- up blocks ------------------------------------------------------------------------------------------
  for (int b = 0; b < nb; ++b) {
    for (auto& r : f->up[b]) TDV_TRY(resnet(f, s, r, H, W));
    if (f->ups_w[b]) {   // Upsample2D: nearest 2x + conv3x3, fused; output replaces X via T1
      const int co = f->up[b][0].cout;
      H *= 2; W *= 2;
      TDV_TRY(conv3(s, f->X, f->ups_w[b], f->ups_b[b], nullptr, f->T1, H, W, co, co, 1));
      std::swap(f->X, f->T1);
    }
  }
  const int clast = f->cfg.block_out_channels[0];
  TDV_TRY(gn(f, s, f->X, f->T1, H * W, clast, f->nout_w, f->nout_b, 1));
  TDV_TRY(conv3(s, f->T1, f->cout_w, f->cout_b, nullptr, f->T2, H, W, clast, f->out_pad, 0));
  TDV_TRY(td_image_finalize_launch(f->T2, H * W, f->out_pad, (unsigned char*)image_u8, (bf16_t*)image_chw, s));
  return TD_OK;
}

}  // extern "C"
