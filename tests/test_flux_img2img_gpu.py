"""FLUX image-to-image (FluxImg2ImgPipelineRewritePrompt) on the GPU: tiny transformer (oracle/flux_ref.tiny_config), full FLUX.1 VAE
architecture with seeded weights (the pipeline's latent size assumes the factor 8 of four blocks).  CPU comparisons use 128 x 128
images (16 x 16 latents); GPU-only checks use 256 x 256.  Bars: latents rel-RMSE < 2e-2 (as test_denoise_loop_matches_oracle),
uint8 pixel RMSE < 1e-2 on the [0, 1] scale; the schedule and batching checks are bit-exact."""
import pytest
import torch

from oracle import flux_ref as R
from oracle import vae_ref as V
from vae_encoder_common import encode_ref, encoder_init_weights, latents_ref, preprocess_u8

pytestmark = pytest.mark.gpu

SCALING, SHIFT = 0.3611, 0.1159


def _rel_rmse(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def setup():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from thinkdiff.models.flux_img2img import FluxImg2ImgPipelineRewritePrompt
    from thinkdiff.models.flux_prompt import FluxPipelineRewritePrompt
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder, AutoencoderKLEncoder
    fc = R.tiny_config(num_layers=1, num_single_layers=1)
    sd_tr = R.init_weights(fc, seed=4)
    tr = FluxTransformer2DModel(FluxTransformerConfig(
        in_channels=fc.in_channels, num_layers=1, num_single_layers=1, num_attention_heads=fc.num_attention_heads,
        joint_attention_dim=fc.joint_attention_dim, pooled_projection_dim=fc.pooled_projection_dim, guidance_embeds=fc.guidance_embeds),
        max_img_tokens=256, max_txt_tokens=128, max_steps=8)
    tr.load_state_dict(sd_tr)
    vcfg = V.VaeConfig()
    sd_dec, sd_enc = V.init_weights(vcfg, seed=12), encoder_init_weights(vcfg, seed=13)
    dec = AutoencoderKLDecoder(AutoencoderKLConfig(), max_latent_size=(32, 32))
    dec.load_state_dict(sd_dec)
    enc = AutoencoderKLEncoder(AutoencoderKLConfig(), max_image_size=(256, 256))
    enc.load_state_dict(sd_enc)
    t2i = FluxPipelineRewritePrompt(transformer=tr, vae=dec)
    i2i = FluxImg2ImgPipelineRewritePrompt.from_pipe(t2i, enc)
    g = torch.Generator().manual_seed(21)
    pe = torch.randn(2, 24, fc.joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(2, fc.pooled_projection_dim, generator=g).bfloat16().cuda()
    return dict(fc=fc, sd_tr=sd_tr, vcfg=vcfg, sd_dec=sd_dec, sd_enc=sd_enc, t2i=t2i, i2i=i2i, pe=pe, pool=pool)


def _image(n, seed):
    from PIL import Image
    u8 = torch.randint(0, 256, (n, n, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    # smooth it a little: a photo-like image, not white noise
    u8 = torch.nn.functional.avg_pool2d(u8.permute(2, 0, 1)[None].float(), 5, 1, 2)[0].permute(1, 2, 0).round().to(torch.uint8)
    return Image.fromarray(u8.numpy()), u8


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def test_strength_one_equals_text_to_image(setup):
    """sigma = 1.0 is exact in bf16, so scale_noise returns the noise: img2img at strength 1 is text-to-image from pack(noise)."""
    s = setup
    img, _ = _image(128, 1)
    kw = dict(prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=128, width=128, num_inference_steps=4, guidance_scale=3.5)
    out = s["i2i"](image=img, strength=1.0, generator=_gen(5), output_type="latent", **kw).images
    g = _gen(5)
    torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=torch.bfloat16)          # the posterior's eps comes first
    noise = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=torch.bfloat16)
    lat = R.pack_latents(noise.cpu()).cuda()
    ref = s["t2i"](latents=lat, output_type="latent", **kw).images
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    out_u8 = s["i2i"](image=img, strength=1.0, generator=_gen(5), output_type="np", **kw).images
    ref_u8 = s["t2i"](latents=lat, output_type="np", **kw).images
    assert torch.equal(out_u8, ref_u8)


def test_img2img_matches_cpu_loop(setup):
    """strength 0.6, 8 steps, 128 x 128: encode, sample, shift / scale, scale_noise, the Euler loop over sigmas[t_start:] and the
    decode, all restated on the CPU."""
    from thinkdiff.models.flux_img2img import get_timesteps
    s = setup
    fc, N, n = s["fc"], 8, 128
    img, u8 = _image(n, 2)
    out = s["i2i"](image=img, strength=0.6, prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=n, width=n,
                   num_inference_steps=N, guidance_scale=3.5, generator=_gen(7), output_type="latent").images
    px = s["i2i"](image=img, strength=0.6, prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=n, width=n,
                  num_inference_steps=N, guidance_scale=3.5, generator=_gen(7), output_type="np").images
    g = _gen(7)
    eps = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=torch.bfloat16).cpu()
    noise = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=torch.bfloat16).cpu()
    t_start = get_timesteps(N, 0.6)
    sig = R.make_sigmas(N, 64)
    mom = encode_ref(s["sd_enc"], s["vcfg"], preprocess_u8(u8))
    x = latents_ref(mom, eps, noise, float(sig[t_start]), SCALING, SHIFT)
    pe, pool = s["pe"][:1].cpu(), s["pool"][:1].cpu()
    img_ids = R.latent_image_ids(8, 8).bfloat16()
    txt_ids = torch.zeros(pe.shape[1], 3).bfloat16()
    guidance = torch.full([1], 3.5, dtype=torch.float32) if fc.guidance_embeds else None
    sig_t = torch.from_numpy(sig)
    for i in range(t_start, N):
        t = (sig_t[i] * 1000.0).expand(1).bfloat16()
        v = R.transformer_forward(s["sd_tr"], fc, x, pe, pool, t / 1000, img_ids, txt_ids, guidance)
        x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
    _, ref_u8 = V.latents_to_image(s["sd_dec"], s["vcfg"], x, 16, 16)
    rel = _rel_rmse(out[0], x[0])
    prmse = float(((px[0].float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"img2img 128x128 strength 0.6, {N - t_start} steps: latents rel-RMSE {rel:.4f}, pixel RMSE {prmse:.5f}")
    assert rel < 2e-2 and prmse < 1e-2


@pytest.mark.parametrize("strength", [0.6, 0.3])
def test_truncated_schedule(setup, strength):
    """The loop runs sigmas[t_start:] of the text-to-image schedule, from the start latents img2img builds: set_timesteps + denoise by
    hand gives the same bits."""
    from thinkdiff.models.flux_img2img import get_timesteps
    from thinkdiff.models.flux_transformer import effective_scalar
    from thinkdiff.models.flux_vae import DiagonalGaussianDistribution
    s = setup
    N, n = 8, 256
    img, _ = _image(n, 3)
    kw = dict(prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=n, width=n, num_inference_steps=N, guidance_scale=3.5)
    out = s["i2i"](image=img, strength=strength, generator=_gen(9), output_type="latent", **kw).images
    t_start = get_timesteps(N, strength)
    sig = s["i2i"].scheduler.sigmas(N, 256)[t_start:]
    g = _gen(9)
    eps = torch.randn((1, 16, 32, 32), generator=g, device="cuda", dtype=torch.bfloat16)
    noise = torch.randn((1, 16, 32, 32), generator=g, device="cuda", dtype=torch.bfloat16)
    enc = s["i2i"].vae_encoder
    _, u8 = _image(n, 3)
    dist = DiagonalGaussianDistribution([enc.encode_moments(u8.cuda())], 32, 32)
    x = dist.packed_latents(0, eps[0], noise[0], float(sig[0]), SCALING, SHIFT)
    tr = s["t2i"].transformer
    tr.set_condition(s["pe"][0], s["pool"][0], R.latent_image_ids(16, 16).cuda(), torch.zeros(s["pe"].shape[1], 3, device="cuda", dtype=torch.bfloat16))
    g_eff = float((torch.tensor([3.5]).bfloat16() * 1000).float()) if tr.config.guidance_embeds else 0.0
    tr.set_timesteps([effective_scalar(float(v) * 1000.0, tr.dtype) for v in sig[:-1]], g_eff)
    tr.denoise(x, sig)
    torch.cuda.synchronize()
    assert len(sig) - 1 == N - t_start
    assert torch.equal(out[0].view(torch.int16), x.view(torch.int16))


def test_given_latents_ignore_the_image(setup):
    s = setup
    kw = dict(prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=256, width=256, num_inference_steps=4,
              guidance_scale=3.5, strength=0.5, output_type="latent")
    lat = torch.randn(1, 256, 64, generator=torch.Generator().manual_seed(1)).bfloat16().cuda()
    a = s["i2i"](image=_image(256, 4)[0], latents=lat, **kw).images
    b = s["i2i"](image=_image(256, 5)[0], latents=lat, **kw).images
    c = s["i2i"](image=None, latents=lat, **kw).images
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(a.view(torch.int16), c.view(torch.int16))
    assert torch.equal(lat.view(torch.int16), torch.randn(1, 256, 64, generator=torch.Generator().manual_seed(1)).bfloat16().cuda().view(torch.int16))


def test_images_in_flight_bit_identical(setup):
    s = setup
    imgs = [_image(256, 6)[0], _image(256, 7)[0]]
    kw = dict(image=imgs, prompt_embeds=s["pe"], pooled_prompt_embeds=s["pool"], height=256, width=256, num_inference_steps=4,
              guidance_scale=3.5, strength=0.6, num_images_per_prompt=2, output_type="latent")
    p = s["i2i"]
    old = p.images_in_flight
    try:
        p.images_in_flight = 2
        two = p(generator=_gen(11), **kw).images
        p.images_in_flight = 1
        one = p(generator=_gen(11), **kw).images
    finally:
        p.images_in_flight = old
    assert two.shape == (4, 256, 64)
    assert torch.equal(two.view(torch.int16), one.view(torch.int16))
    assert not torch.equal(two[0], two[1])       # different noise per sample


def test_aligner_shaped_prompt_embeds(setup):
    """T = 128 prompt tokens (the aligner's output shape), no text encoders loaded."""
    s = setup
    g = torch.Generator().manual_seed(31)
    pe = torch.randn(1, 128, s["fc"].joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(1, s["fc"].pooled_projection_dim, generator=g).bfloat16().cuda()
    out = s["i2i"](image=_image(256, 8)[0], prompt_embeds=pe, pooled_prompt_embeds=pool, height=256, width=256, num_inference_steps=4,
                   guidance_scale=3.5, strength=0.6, generator=_gen(1))
    im = out.images[0]
    assert im.size == (256, 256) and im.mode == "RGB"
