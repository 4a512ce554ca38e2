"""FLUX inpainting (FluxInpaintPipelineRewritePrompt, flux_inpaint_step_, flux_inpaint_mask, flux_denoise_inpaint_) on the GPU: tiny
transformer (oracle/flux_ref.tiny_config) and the full FLUX.1 VAE architecture with seeded weights, as test_flux_img2img_gpu.py
builds them.  The kernels and the engine loop are bit-exact with the eager torch statements of the spec (thinkdiff/models/
flux_inpaint.py); the CPU loop at 128 x 128 uses the img2img bars (latents rel-RMSE < 2e-2, pixel RMSE < 1e-2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import flux_ref as R
from oracle import vae_ref as V
from vae_encoder_common import encode_ref, encoder_init_weights, latents_ref, preprocess_u8

pytestmark = pytest.mark.gpu

SCALING, SHIFT = 0.3611, 0.1159
BF = torch.bfloat16


def _ops():
    from thinkdiff.ops import register
    return register()


def _i16(t):
    return t.contiguous().view(torch.int16)


def _rel_rmse(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def step_ref(x, v, z, noise, m, dt, sigma_next):
    """The spec's step 4 as the diffusers statements, eager torch on bf16 tensors (scheduler.step, scale_noise, the blend)."""
    dt_t = torch.tensor(dt, dtype=torch.float32, device=x.device)
    a = (x.to(torch.float32) + dt_t * v).to(v.dtype)
    if noise is None:
        p = z
    else:
        s = torch.tensor([sigma_next], dtype=torch.float32, device=x.device).to(BF)[:, None]
        p = s * noise + (1.0 - s) * z
    return (1 - m) * p + m * a


def mask_ref(mask, C=16):
    """mask_processor's binarize, prepare_mask_latents' F.interpolate(nearest) / repeat / _pack_latents: [H, W] -> [S, 4C] bf16."""
    m = mask.float() / 255 if mask.dtype == torch.uint8 else mask.clone()
    m[m < 0.5] = 0
    m[m >= 0.5] = 1
    H, W = m.shape
    m = F.interpolate(m[None, None], size=(H // 8, W // 8)).to(BF)
    return R.pack_latents(m.repeat(1, C, 1, 1))[0]


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from thinkdiff.models.flux_inpaint import FluxInpaintPipelineRewritePrompt
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
    inp = FluxInpaintPipelineRewritePrompt.from_pipe(t2i, enc)
    g = torch.Generator().manual_seed(21)
    pe = torch.randn(2, 24, fc.joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(2, fc.pooled_projection_dim, generator=g).bfloat16().cuda()
    return dict(fc=fc, sd_tr=sd_tr, vcfg=vcfg, sd_dec=sd_dec, sd_enc=sd_enc, t2i=t2i, i2i=i2i, inp=inp, pe=pe, pool=pool)


def _image(n, seed):
    from PIL import Image
    u8 = torch.randint(0, 256, (n, n, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    u8 = F.avg_pool2d(u8.permute(2, 0, 1)[None].float(), 5, 1, 2)[0].permute(1, 2, 0).round().to(torch.uint8)
    return Image.fromarray(u8.numpy()), u8


def _mask(n, kind):
    """PIL "L" masks: 255 = repaint.  left / top: that half of the picture."""
    from PIL import Image
    a = np.zeros((n, n), np.uint8)
    if kind == "ones":
        a[:] = 255
    elif kind == "left":
        a[:, : n // 2] = 255
    elif kind == "top":
        a[: n // 2] = 255
    return Image.fromarray(a, "L")


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _clean_latents(s, imgs_u8, generator_seed, n_img):
    """z_i the pipeline blends with: the posterior sample with the call's first draw (eps), shift / scale, packed."""
    from thinkdiff.models.flux_vae import DiagonalGaussianDistribution
    h = imgs_u8[0].shape[0] // 8
    eps = torch.randn((n_img, 16, h, h), generator=_gen(generator_seed), device="cuda", dtype=BF)
    enc = s["inp"].vae_encoder
    dist = DiagonalGaussianDistribution([enc.encode_moments(u.cuda()) for u in imgs_u8], h, h)
    return [dist.packed_latents(i, eps[i], None, 0.0, SCALING, SHIFT) for i in range(n_img)]


@pytest.mark.parametrize("sigma", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("mask_kind", ["binary", "fractional", "zeros", "ones"])
def test_inpaint_step_bit_exact(sigma, with_noise, mask_kind):
    S = 1024
    g = torch.Generator().manual_seed(int(sigma * 10) + 3 * with_noise + len(mask_kind))
    x, v, z, noise = ((torch.randn(S, 64, generator=g) * sc).to(BF).cuda() for sc in (1.0, 1.3, 0.8, 1.0))
    m = {"binary": (torch.rand(S, 64, generator=g) < 0.5).float(), "fractional": torch.rand(S, 64, generator=g),
         "zeros": torch.zeros(S, 64), "ones": torch.ones(S, 64)}[mask_kind].to(BF).cuda()
    s_cur = np.float32(min(sigma + 0.0714, 1.0)) if sigma < 1.0 else np.float32(1.0)
    dt = float(np.float32(sigma) - s_cur) if sigma < 1.0 else -0.0357
    nz = noise if with_noise else None
    want = step_ref(x, v, z, nz, m, dt, sigma)
    got = x.clone()
    _ops().flux_inpaint_step_(got, v, z, nz, m, dt, sigma)
    torch.cuda.synchronize()
    assert torch.equal(_i16(got), _i16(want))


@pytest.mark.parametrize("H,W", [(128, 128), (256, 384), (1024, 1024)])
@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_inpaint_mask_bit_exact(H, W, fmt):
    g = torch.Generator().manual_seed(H + W)
    if fmt == "u8":
        src = torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8)
        edge = torch.tensor([127, 128, 0, 255], dtype=torch.uint8)
    else:
        src = torch.rand(H, W, generator=g)
        edge = torch.tensor([0.5, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.0, 1.0])
    # the thresholds at sampled pixels (8y, 8x): the ones the nearest interpolation reads
    for k, (y, x) in enumerate([(0, 0), (8, 16), (H - 8, W - 8), (16, 0), (8, 8), (H // 2, W // 2), (0, 8), (24, 40)]):
        src[y, x] = edge[k % 4]
    want = mask_ref(src)
    got = _ops().flux_inpaint_mask(src.cuda(), 16)
    torch.cuda.synchronize()
    assert got.shape == ((H // 16) * (W // 16), 64)
    assert torch.equal(_i16(got.cpu()), _i16(want))
    assert 0 < float(want.float().mean()) < 1


def _prepared(s, n, N, strength, prompt=0):
    from thinkdiff.models.flux_img2img import get_timesteps
    from thinkdiff.models.flux_transformer import effective_scalar
    t_start = get_timesteps(N, strength)
    sig = s["inp"].scheduler.sigmas(N, (n // 16) ** 2)[t_start:]
    tr = s["t2i"].transformer
    tr.set_condition(s["pe"][prompt], s["pool"][prompt], R.latent_image_ids(n // 16, n // 16).cuda(),
                     torch.zeros(s["pe"].shape[1], 3, device="cuda", dtype=BF))
    g_eff = float((torch.tensor([3.5]).bfloat16() * 1000).float()) if tr.config.guidance_embeds else 0.0
    tr.set_timesteps([effective_scalar(float(v) * 1000.0, tr.dtype) for v in sig[:-1]], g_eff)
    return tr, sig


def test_engine_loop_matches_forward_and_eager_step(setup):
    """td_flux_denoise_inpaint at 256 x 256, 8 steps, strength 0.6 (5 steps) = forward_step + the eager step-4 statements, step by step."""
    s = setup
    tr, sig = _prepared(s, 256, 8, 0.6)
    g = torch.Generator().manual_seed(5)
    x0, z, noise = (torch.randn(256, 64, generator=g).to(BF).cuda() for _ in range(3))
    mask = mask_ref(torch.randint(0, 256, (256, 256), generator=g, dtype=torch.uint8)).cuda()
    ref = x0.clone()
    n = len(sig) - 1
    for i in range(n):
        v = tr.forward_step(ref, i)
        ref = step_ref(ref, v, z, noise if i < n - 1 else None, mask, float(np.float32(sig[i + 1]) - np.float32(sig[i])), float(sig[i + 1]))
    x = x0.clone()
    tr.denoise(x, sig, inpaint=(z, noise, mask))
    torch.cuda.synchronize()
    assert n == 5 and torch.equal(_i16(x), _i16(ref))
    # the blend buffers must not alias the latents the loop writes
    with pytest.raises(RuntimeError, match="overlap"):
        tr.denoise(x, sig, inpaint=(z, x, mask))


def test_inpaint_matches_cpu_loop(setup):
    """strength 0.6, 8 steps, 128 x 128, left half repainted: encode, sample, scale_noise, the Euler loop with the blend and the decode,
    all restated on the CPU."""
    from thinkdiff.models.flux_img2img import get_timesteps
    s = setup
    fc, N, n = s["fc"], 8, 128
    img, u8 = _image(n, 2)
    mk = _mask(n, "left")
    kw = dict(image=img, mask_image=mk, strength=0.6, prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=n, width=n,
              num_inference_steps=N, guidance_scale=3.5)
    out = s["inp"](generator=_gen(7), output_type="latent", **kw).images
    px = s["inp"](generator=_gen(7), output_type="np", **kw).images
    g = _gen(7)
    eps = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
    noise = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
    t_start = get_timesteps(N, 0.6)
    sig = R.make_sigmas(N, 64)
    mom = encode_ref(s["sd_enc"], s["vcfg"], preprocess_u8(u8))
    z = latents_ref(mom, eps, None, 0.0, SCALING, SHIFT)
    x = latents_ref(mom, eps, noise, float(sig[t_start]), SCALING, SHIFT)
    noise_p = R.pack_latents(noise)
    m = mask_ref(torch.from_numpy(np.array(mk)))[None]
    pe, pool = s["pe"][:1].cpu(), s["pool"][:1].cpu()
    img_ids = R.latent_image_ids(8, 8).bfloat16()
    txt_ids = torch.zeros(pe.shape[1], 3).bfloat16()
    guidance = torch.full([1], 3.5, dtype=torch.float32) if fc.guidance_embeds else None
    sig_t = torch.from_numpy(sig)
    for i in range(t_start, N):
        t = (sig_t[i] * 1000.0).expand(1).bfloat16()
        v = R.transformer_forward(s["sd_tr"], fc, x, pe, pool, t / 1000, img_ids, txt_ids, guidance)
        x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
        if i < N - 1:
            sb = sig_t[i + 1:i + 2].to(BF)[:, None, None]
            p = sb * noise_p + (1.0 - sb) * z
        else:
            p = z
        x = (1 - m) * p + m * x
    _, ref_u8 = V.latents_to_image(s["sd_dec"], s["vcfg"], x, 16, 16)
    rel = _rel_rmse(out[0], x[0])
    prmse = float(((px[0].float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"inpaint 128x128 strength 0.6, {N - t_start} steps: latents rel-RMSE {rel:.4f}, pixel RMSE {prmse:.5f}")
    assert rel < 2e-2 and prmse < 1e-2


def test_all_ones_mask_is_img2img(setup):
    """m = 1 everywhere: x' = bf16(0 * p) + a = a in value (the sign of a zero may differ); the extra draw comes after img2img's."""
    s = setup
    img, _ = _image(128, 3)
    kw = dict(image=img, strength=0.6, prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=128, width=128,
              num_inference_steps=6, guidance_scale=3.5)
    a = s["inp"](mask_image=_mask(128, "ones"), generator=_gen(3), output_type="latent", **kw).images
    b = s["i2i"](generator=_gen(3), output_type="latent", **kw).images
    assert torch.equal(a.float(), b.float())
    a = s["inp"](mask_image=_mask(128, "ones"), generator=_gen(3), output_type="np", **kw).images
    b = s["i2i"](generator=_gen(3), output_type="np", **kw).images
    assert torch.equal(a, b)


@pytest.mark.parametrize("strength", [0.6, 1.0])
def test_all_zeros_mask_returns_clean_latents(setup, strength):
    s = setup
    img, u8 = _image(128, 4)
    out = s["inp"](image=img, mask_image=_mask(128, "zeros"), strength=strength, prompt_embeds=s["pe"][:1],
                   pooled_prompt_embeds=s["pool"][:1], height=128, width=128, num_inference_steps=6, guidance_scale=3.5,
                   generator=_gen(4), output_type="latent").images
    z = _clean_latents(s, [u8], 4, 1)[0]
    assert torch.equal(out[0].float(), z.float())


def _masked_tokens(n, kind):
    return mask_ref(torch.from_numpy(np.array(_mask(n, kind))))[:, 0].bool().cuda()


def test_half_mask_keeps_the_unmasked_tokens(setup):
    s = setup
    img, u8 = _image(256, 5)
    out = s["inp"](image=img, mask_image=_mask(256, "left"), strength=0.6, prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1],
                   height=256, width=256, num_inference_steps=6, guidance_scale=3.5, generator=_gen(5), output_type="latent").images[0]
    z = _clean_latents(s, [u8], 5, 1)[0]
    on = _masked_tokens(256, "left")
    assert 0 < int(on.sum()) < on.numel()
    assert torch.equal(out[~on].float(), z[~on].float())
    assert not torch.equal(out[on].float(), z[on].float())


def test_images_in_flight_and_mask_per_sample(setup):
    """2 prompts x 2 images per prompt, two images and two masks: sample b takes image b % 2 and mask b % 2; two in flight and one at
    a time give the same bits."""
    s = setup
    (i0, u0), (i1, u1) = _image(256, 6), _image(256, 7)
    kw = dict(image=[i0, i1], mask_image=[_mask(256, "left"), _mask(256, "top")], prompt_embeds=s["pe"], pooled_prompt_embeds=s["pool"],
              height=256, width=256, num_inference_steps=4, guidance_scale=3.5, strength=0.6, num_images_per_prompt=2, output_type="latent")
    p = s["inp"]
    old = p.images_in_flight
    try:
        p.images_in_flight = 2
        two = p(generator=_gen(11), **kw).images
        p.images_in_flight = 1
        one = p(generator=_gen(11), **kw).images
    finally:
        p.images_in_flight = old
    assert two.shape == (4, 256, 64)
    assert torch.equal(_i16(two), _i16(one))
    z = _clean_latents(s, [u0, u1], 11, 2)
    masks = [_masked_tokens(256, "left"), _masked_tokens(256, "top")]
    for b in range(4):
        on = masks[b % 2]
        assert torch.equal(two[b][~on].float(), z[b % 2][~on].float()), b
        assert not torch.equal(two[b][on].float(), z[b % 2][on].float()), b
        # the other mask's unmasked region (where it differs from this one) is repainted
        other = masks[1 - b % 2]
        assert not torch.equal(two[b][~other & on].float(), z[b % 2][~other & on].float()), b


def test_given_unpacked_latents_are_start_and_noise(setup):
    s = setup
    img, u8 = _image(256, 8)
    mk = _mask(256, "left")
    lat = torch.randn(1, 16, 32, 32, generator=torch.Generator().manual_seed(1)).to(BF).cuda()
    keep = lat.clone()
    out = s["inp"](image=img, mask_image=mk, latents=lat, strength=0.6, prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1],
                   height=256, width=256, num_inference_steps=8, guidance_scale=3.5, generator=_gen(12), output_type="latent").images[0]
    assert torch.equal(_i16(lat), _i16(keep))                   # the caller's tensor is not written
    z = _clean_latents(s, [u8], 12, 1)[0]
    tr, sig = _prepared(s, 256, 8, 0.6)
    noise = R.pack_latents(lat)[0].contiguous()
    x = noise.clone()
    tr.denoise(x, sig, inpaint=(z, noise, mask_ref(torch.from_numpy(np.array(mk))).cuda()))
    torch.cuda.synchronize()
    assert torch.equal(_i16(out), _i16(x))
    on = _masked_tokens(256, "left")
    assert torch.equal(out[~on].float(), z[~on].float())


@pytest.mark.parametrize("case", ["default", "latents", "masked_image_latents", "two_masks"])
def test_generator_position_after_a_call(setup, case):
    """eps [B_img], then noise [B] (not with latents=), then the dropped draw [max(B_img, B_m)] (not with 16-channel masked_image_latents)."""
    s = setup
    img, _ = _image(128, 9)
    kw = dict(image=img, mask_image=_mask(128, "left"), strength=0.6, prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1],
              height=128, width=128, num_inference_steps=4, guidance_scale=3.5, output_type="latent")
    n_masks = 1
    if case == "latents":
        kw["latents"] = torch.zeros(1, 16, 16, 16, dtype=BF, device="cuda")
    elif case == "masked_image_latents":
        kw["masked_image_latents"] = torch.zeros(1, 16, 16, 16, dtype=BF, device="cuda")
    elif case == "two_masks":
        kw["mask_image"] = [_mask(128, "left"), _mask(128, "top")]
        kw["num_images_per_prompt"] = 2
        n_masks = 2
    B = kw.get("num_images_per_prompt", 1)
    g = _gen(13)
    s["inp"](generator=g, **kw)
    after = torch.randn(64, generator=g, device="cuda", dtype=BF)
    r = _gen(13)
    torch.randn((1, 16, 16, 16), generator=r, device="cuda", dtype=BF)
    if case != "latents":
        torch.randn((B, 16, 16, 16), generator=r, device="cuda", dtype=BF)
    if case != "masked_image_latents":
        torch.randn((max(1, n_masks), 16, 16, 16), generator=r, device="cuda", dtype=BF)
    want = torch.randn(64, generator=r, device="cuda", dtype=BF)
    assert torch.equal(_i16(after), _i16(want))


def test_pil_output_and_aligner_shaped_prompt(setup):
    s = setup
    g = torch.Generator().manual_seed(31)
    pe = torch.randn(1, 128, s["fc"].joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(1, s["fc"].pooled_projection_dim, generator=g).bfloat16().cuda()
    m = torch.zeros(256, 256)
    m[64:192, 64:192] = 1.0
    out = s["inp"](image=_image(256, 10)[0], mask_image=m, prompt_embeds=pe, pooled_prompt_embeds=pool, height=256, width=256,
                   num_inference_steps=4, guidance_scale=3.5, strength=0.6, generator=_gen(1))
    im = out.images[0]
    assert im.size == (256, 256) and im.mode == "RGB"
