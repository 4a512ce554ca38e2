"""Channel-conditioned FLUX on the GPU (FLUX.1 Fill: in 384 / out 64; FLUX.1 Canny / Depth: in 128 / out 64): tiny transformers
(oracle/flux_ref.tiny_config, 1 + 1 blocks) and the full FLUX.1 VAE architecture with seeded weights, as test_flux_inpaint_gpu.py
builds them.  The conditioning kernels are bit-exact with the eager torch statements of the spec (thinkdiff/models/flux_fill.py,
tests/fill_common.py); the conditioned forward is held to test_flux_engine_gpu.py's bars (bf16 oracle rel-RMSE < 2e-2, fp32 oracle
< 1.5 e_ref + 2e-3), the 8-bit modes to test_fp8_mode_matches_fp8_oracle's and test_int8_gpu.py's, the pipelines at 128 x 128 to the
img2img bars (latents rel-RMSE < 2e-2, pixel RMSE < 1e-2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fill_common import (LAT, build_engine, conditioned_weights, denoise_ref, fill_condition_ref, forward_ref, masked_image_ref,
                         preprocess_f32, unshuffle_ref)
from oracle import flux_ref as R
from oracle import vae_ref as V
from vae_encoder_common import encode_ref, encoder_init_weights, latents_ref, nhwc_moments_to_nchw, preprocess_u8

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


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _image(n, seed):
    from PIL import Image
    u8 = torch.randint(0, 256, (n, n, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    u8 = F.avg_pool2d(u8.permute(2, 0, 1)[None].float(), 5, 1, 2)[0].permute(1, 2, 0).round().to(torch.uint8)
    return Image.fromarray(u8.numpy()), u8


def _mask(n, kind):
    """PIL "L" masks: 255 = fill.  left / top: that half of the picture; blob: an off-grid rectangle (its edges cut through 8 x 8 blocks)."""
    from PIL import Image
    a = np.zeros((n, n), np.uint8)
    if kind == "ones":
        a[:] = 255
    elif kind == "left":
        a[:, : n // 2] = 255
    elif kind == "top":
        a[: n // 2] = 255
    elif kind == "blob":
        a[n // 4 + 3: n // 2 + 5, n // 8 + 1: n - 13] = 255
    return Image.fromarray(a, "L")


def _mask_t(n, kind):
    return torch.from_numpy(np.array(_mask(n, kind)))


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from thinkdiff.models import FluxControlPipelineRewritePrompt, FluxFillPipelineRewritePrompt
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder, AutoencoderKLEncoder
    s = {}
    for name, c_in, seed in (("fill", 384, 4), ("ctrl", 128, 5)):
        cfg, sd, eng = conditioned_weights(c_in, seed)
        s[name] = dict(cfg=cfg, sd=sd, eng=eng, tr=build_engine(cfg, eng))
    vcfg = V.VaeConfig()
    sd_dec, sd_enc = V.init_weights(vcfg, seed=12), encoder_init_weights(vcfg, seed=13)
    dec = AutoencoderKLDecoder(AutoencoderKLConfig(), max_latent_size=(32, 32))
    dec.load_state_dict(sd_dec)
    enc = AutoencoderKLEncoder(AutoencoderKLConfig(), max_image_size=(256, 256))
    enc.load_state_dict(sd_enc)
    s["fill"]["pipe"] = FluxFillPipelineRewritePrompt(transformer=s["fill"]["tr"], vae=dec, vae_encoder=enc)
    s["ctrl"]["pipe"] = FluxControlPipelineRewritePrompt(transformer=s["ctrl"]["tr"], vae=dec, vae_encoder=enc)
    fc = s["fill"]["cfg"]
    g = torch.Generator().manual_seed(21)
    s.update(vcfg=vcfg, sd_dec=sd_dec, sd_enc=sd_enc, enc=enc,
             pe=torch.randn(2, 24, fc.joint_attention_dim, generator=g).bfloat16().cuda(),
             pool=torch.randn(2, fc.pooled_projection_dim, generator=g).bfloat16().cuda())
    return s


# ---- conditioning kernels: bit-exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(128, 128), (64, 96)])
@pytest.mark.parametrize("img_fmt", ["u8", "f32"])
@pytest.mark.parametrize("mask_kind", ["random_u8", "random_f32", "zeros", "ones"])
def test_masked_image_in_bit_exact(hip, H, W, img_fmt, mask_kind):
    """The image-in stage of td_vae_encode_masked against (preprocess(image) * (1 - m)).to(bf16).  All-zeros = td_vae_image_to_nhwc_bf16;
    all-ones = zero everywhere (each zero carries the sign of 2x - 1, as the fp32 product does, so the bits are compared as well)."""
    g = torch.Generator().manual_seed(H + W + len(mask_kind))
    u8 = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    if img_fmt == "u8":
        img, x = u8, preprocess_f32(u8)
    else:
        img = torch.rand(3, H, W, generator=g)
        x = (2 * img - 1)[None]
    if mask_kind == "random_u8":
        mask = torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8)
        mask[0, :4] = torch.tensor([127, 128, 0, 255], dtype=torch.uint8)
    elif mask_kind == "random_f32":
        mask = torch.rand(H, W, generator=g)
        mask[0, :4] = torch.tensor([0.5, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.0, 1.0])
    else:
        mask = torch.full((H, W), 255 if mask_kind == "ones" else 0, dtype=torch.uint8)
    want = masked_image_ref(x, mask)[0].permute(1, 2, 0).reshape(H * W, 3)
    got = hip.vae_image_to_nhwc(img.cuda(), 64, mask=mask.cuda())
    torch.cuda.synchronize()
    assert got.shape == (H * W, 64)
    assert torch.equal(_i16(got[:, :3].cpu()), _i16(want))
    assert not got[:, 3:].any()
    if mask_kind == "zeros":
        assert torch.equal(_i16(got), _i16(hip.vae_image_to_nhwc(img.cuda(), 64)))
    if mask_kind == "ones":
        assert not (got.float() != 0).any()


@pytest.mark.parametrize("H,W", [(128, 128), (64, 96), (256, 256)])
@pytest.mark.parametrize("mask_fmt", ["u8", "f32"])
@pytest.mark.parametrize("with_eps", [True, False])
def test_fill_condition_bit_exact(hip, H, W, mask_fmt, with_eps):
    """flux_fill_condition against eager torch: latents_ref (sample or mode, shift / scale, pack) | the unshuffle restatement."""
    g = torch.Generator().manual_seed(H * 3 + W + with_eps)
    h, w = H // 8, W // 8
    mom = torch.cat([torch.randn(1, 16, h, w, generator=g), torch.randn(1, 16, h, w, generator=g) * 3 - 2], dim=1).to(BF)
    mom[0, 16, 0, 0], mom[0, 17, 0, 0] = 40.0, -50.0                     # the logvar clamp
    eps = torch.randn(1, 16, h, w, generator=g).to(BF) if with_eps else None
    if mask_fmt == "u8":
        mask = torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8)
        mask[0, :4] = torch.tensor([127, 128, 0, 255], dtype=torch.uint8)
    else:
        mask = torch.rand(H, W, generator=g)
        mask[0, :4] = torch.tensor([0.5, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.0, 1.0])
    want = fill_condition_ref(mom, eps, mask, SCALING, SHIFT)
    mom_nhwc = mom[0].permute(1, 2, 0).reshape(h * w, 32).contiguous().cuda()
    got = _ops().flux_fill_condition(mom_nhwc, None if eps is None else eps[0].contiguous().cuda(), mask.cuda(), SCALING, SHIFT, H, W)
    torch.cuda.synchronize()
    assert got.shape == ((H // 16) * (W // 16), 320)
    assert torch.equal(_i16(got.cpu()[:, :LAT]), _i16(want[:, :LAT]))
    assert torch.equal(_i16(got.cpu()[:, LAT:]), _i16(want[:, LAT:]))
    # the latent columns are td_vae_latents_from_moments', the mask columns hold every pixel once
    lat = _ops().vae_latents_from_moments(mom_nhwc, None if eps is None else eps[0].contiguous().cuda(), None, 0.0, SCALING, SHIFT, h, w)
    assert torch.equal(_i16(got[:, :LAT]), _i16(lat))
    assert int(got[:, LAT:].float().sum()) == int((unshuffle_ref(mask).float()).sum())


def test_masked_encode_matches_encoder_on_masked_image(setup):
    """td_vae_encode_masked = td_vae_encode's network behind the masked image-in stage: all-zeros mask gives td_vae_encode's bits, a half
    mask gives the CPU encoder's moments of the masked image at test_vae_encoder_gpu.py's bar (moments rel-RMSE < 3e-2)."""
    s = setup
    _, u8 = _image(128, 2)
    enc = s["enc"]
    plain = enc.encode_moments(u8)
    zero = enc.encode_moments(u8, mask=_mask_t(128, "zeros"))
    half = enc.encode_moments(u8, mask=_mask_t(128, "left"))
    torch.cuda.synchronize()
    assert torch.equal(_i16(plain), _i16(zero)) and not torch.equal(_i16(plain), _i16(half))
    ref = encode_ref(s["sd_enc"], s["vcfg"], masked_image_ref(preprocess_f32(u8), _mask_t(128, "left")))
    e = _rel_rmse(nhwc_moments_to_nchw(half.cpu(), 16, 16), ref)
    print(f"masked encode 128x128: moments rel-RMSE vs the CPU encoder {e:.4f}")
    assert e < 3e-2


# ---- the conditioned forward -----------------------------------------------------------------------------------------------------------
def _fwd_inputs(cfg, h2, w2, T, seed):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(1, h2 * w2, LAT, generator=g).bfloat16()
    cond = torch.randn(1, h2 * w2, cfg.in_channels - LAT, generator=g).bfloat16()
    pe = torch.randn(1, T, cfg.joint_attention_dim, generator=g).bfloat16()
    pool = torch.randn(1, cfg.pooled_projection_dim, generator=g).bfloat16()
    return lat, cond, pe, pool


@pytest.mark.parametrize("which,h2,w2,T", [("fill", 8, 8, 24), ("fill", 12, 20, 65), ("ctrl", 8, 8, 24), ("ctrl", 12, 20, 65)])
def test_conditioned_forward_matches_oracle(setup, which, h2, w2, T):
    """The diffusers-shaped forward on hidden_states = cat(latents, cond) [1, S, Cin] against the oracle with in_channels = Cin (first 64
    output columns), at test_transformer_forward_matches_oracle's bars; the condition matters."""
    e = setup[which]
    cfg, sd, m = e["cfg"], e["sd"], e["tr"]
    lat, cond, pe, pool = _fwd_inputs(cfg, h2, w2, T, seed=T + cfg.in_channels)
    img_ids, txt_ids = R.latent_image_ids(h2, w2), torch.zeros(T, 3)
    t, g = torch.tensor([0.7324]), torch.tensor([3.5])
    ref16 = forward_ref(sd, cfg, lat, cond, pe, pool, t.bfloat16(), img_ids.bfloat16(), txt_ids.bfloat16(), g)
    sd32 = {k: v.float() for k, v in sd.items()}
    ref32 = forward_ref(sd32, cfg, lat.float(), cond.float(), pe.float(), pool.float(), t.bfloat16().float(), img_ids, txt_ids,
                        torch.tensor([float((g.bfloat16() * 1000).float()) / 1000]))
    hs = torch.cat([lat, cond], dim=2).cuda()
    out = m.forward(hs, pe.cuda(), pool.cuda(), t.bfloat16().cuda(), img_ids, txt_ids, g)[0].clone()
    other = m.forward(torch.cat([lat, cond.flip(1)], dim=2).cuda(), pe.cuda(), pool.cuda(), t.bfloat16().cuda(), img_ids, txt_ids, g)[0]
    torch.cuda.synchronize()
    e16, e32, e_ref, d = _rel_rmse(out, ref16), _rel_rmse(out, ref32), _rel_rmse(ref16, ref32), _rel_rmse(other, out)
    print(f"Cin {cfg.in_channels}: hip~bf16-oracle {e16:.4f}  hip~fp32-oracle {e32:.4f}  bf16-oracle~fp32-oracle {e_ref:.4f}  other condition {d:.4f}")
    assert out.shape == (1, h2 * w2, LAT)
    assert e16 < 2e-2
    assert e32 < 1.5 * e_ref + 2e-3
    assert d > 2e-2                       # another condition moves the output by more than the parity bar itself
    with pytest.raises(ValueError, match="in_channels"):
        m.forward(lat.cuda(), pe.cuda(), pool.cuda(), t.bfloat16().cuda(), img_ids, txt_ids, g)


def _prepare(m, pe, pool, h2, w2, n):
    from thinkdiff.models.flux_transformer import effective_scalar
    sig = R.make_sigmas(n, h2 * w2)
    m.set_condition(pe, pool, R.latent_image_ids(h2, w2))
    m.set_timesteps([effective_scalar(float(v) * 1000.0, BF) for v in sig[:-1]], float((torch.tensor([3.5]).bfloat16() * 1000).float()))
    return sig


def test_zero_condition_reproduces_the_plain_model(setup):
    """Engine A (Cin = 384) with an all-zero condition against engine B (Cin = 64) loaded with x_embedder.weight[:, :64] of A and the rest
    equal.  Zeros add exactly in the fp32 accumulator, so if the GEMM launcher keeps the summation order A equals B bit for bit on a forward
    and on a 4-step denoise; if it picks another tile or kernel for K = 384 and the sums reorder, A must be no further from B than B is from
    the bf16 oracle.  Which of the two held is printed.  On the MI355X the first held: A == B bit for bit, forward and denoise (the launcher
    picks the same tile for K = 64 and K = 384 at these shapes and walks K in order)."""
    e = setup["fill"]
    a = e["tr"]
    cfg_b = R.tiny_config(num_layers=1, num_single_layers=1)
    sd_b = dict(e["eng"])
    sd_b["x_embedder.weight"] = e["eng"]["x_embedder.weight"][:, :LAT].contiguous()
    b = build_engine(cfg_b, sd_b, out_channels=None)
    h2 = w2 = 16
    T, n = 40, 4
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(h2 * w2, LAT, generator=g).bfloat16().cuda()
    pe = torch.randn(T, cfg_b.joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(cfg_b.pooled_projection_dim, generator=g).bfloat16().cuda()
    sig = _prepare(a, pe, pool, h2, w2, n)
    a.set_channel_condition(torch.zeros(h2 * w2, 320, dtype=BF, device="cuda"))
    _prepare(b, pe, pool, h2, w2, n)
    va, vb = a.forward_step(lat, 0).clone(), b.forward_step(lat, 0).clone()
    xa, xb = lat.clone(), lat.clone()
    a.denoise(xa, sig)
    b.denoise(xb, sig)
    torch.cuda.synchronize()
    # the oracle of B: the 64-channel model (proj_out of the 384-channel state dict sliced, which is what both engines hold)
    ref = R.denoise(sd_b, cfg_b, lat[None].cpu(), pe[None].cpu(), pool[None].cpu(), h2, w2, n, guidance_scale=3.5)
    exact = torch.equal(_i16(va), _i16(vb)) and torch.equal(_i16(xa), _i16(xb))
    d_ab, d_b = _rel_rmse(xa, xb), _rel_rmse(xb[None], ref)
    print(f"zero condition: A == B bit for bit: {exact};  A~B {d_ab:.5f}  B~bf16-oracle {d_b:.5f}")
    assert exact or d_ab <= d_b
    assert d_b < 2e-2
    # a non-zero condition moves it
    a.set_channel_condition(torch.ones(h2 * w2, 320, dtype=BF, device="cuda"))
    assert not torch.equal(_i16(a.forward_step(lat, 0)), _i16(vb))


def test_stale_or_missing_channel_condition_is_refused(setup):
    """A forward on a conditioned engine needs a channel condition written for the current token count; an unconditioned engine takes none."""
    e = setup["ctrl"]
    m = e["tr"].fork()                      # a fresh context: nothing set yet
    cfg = e["cfg"]
    g = torch.Generator().manual_seed(1)
    pe = torch.randn(24, cfg.joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(cfg.pooled_projection_dim, generator=g).bfloat16().cuda()
    _prepare(m, pe, pool, 8, 8, 2)
    lat = torch.randn(64, LAT, generator=g).bfloat16().cuda()
    with pytest.raises(RuntimeError, match="condition"):
        m.forward_step(lat, 0)
    with pytest.raises(RuntimeError, match=r"\[64, 64\]"):
        m.set_channel_condition(torch.zeros(16, 64, dtype=BF, device="cuda"))
    m.set_channel_condition(torch.zeros(64, 64, dtype=BF, device="cuda"))
    m.forward_step(lat, 0)
    _prepare(m, pe, pool, 8, 8, 2)          # the same token count: the condition stays
    m.forward_step(lat, 0)
    _prepare(m, pe, pool, 4, 4, 2)          # another S_img: the condition is void
    with pytest.raises(RuntimeError, match="condition"):
        m.forward_step(lat[:16].contiguous(), 0)
    with pytest.raises(RuntimeError, match="condition"):
        m.denoise(lat[:16].contiguous(), R.make_sigmas(2, 16))
    torch.cuda.synchronize()
    from thinkdiff import _hip
    plain = build_engine(R.tiny_config(num_layers=1, num_single_layers=1), R.init_weights(R.tiny_config(num_layers=1, num_single_layers=1), seed=1),
                         out_channels=None)
    with pytest.raises(_hip.ThinkDiffHipError, match="no channel condition"):
        plain.set_channel_condition(torch.zeros(64, 64, dtype=BF, device="cuda"))
    _prepare(plain, pe, pool, 8, 8, 2)
    with pytest.raises(RuntimeError, match="no channel condition"):
        _ops().flux_set_channel_condition(int(plain._h.value), torch.zeros(64, 64, dtype=BF, device="cuda"))


# ---- the pipelines ---------------------------------------------------------------------------------------------------------------------
def _fill_kw(s, n, **over):
    kw = dict(prompt_embeds=s["pe"][:1], pooled_prompt_embeds=s["pool"][:1], height=n, width=n, num_inference_steps=4, guidance_scale=3.5)
    kw.update(over)
    return kw


def test_fill_matches_cpu_loop(setup):
    """128 x 128, 4 steps, an off-grid mask: masked encode, posterior sample, condition, the conditioned Euler loop and the decode, all
    restated on the CPU; noise and eps are drawn from a device generator in the order of the spec (noise first, then eps)."""
    s = setup
    e, n, N = s["fill"], 128, 4
    img, u8 = _image(n, 2)
    mk = _mask(n, "blob")
    kw = _fill_kw(s, n, image=img, mask_image=mk)
    out = e["pipe"](generator=_gen(7), output_type="latent", **kw).images
    px = e["pipe"](generator=_gen(7), output_type="np", **kw).images
    g = _gen(7)
    noise = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
    eps = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
    mask = torch.from_numpy(np.array(mk))
    mom = encode_ref(s["sd_enc"], s["vcfg"], masked_image_ref(preprocess_f32(u8), mask))
    cond = fill_condition_ref(mom, eps, mask, SCALING, SHIFT)[None]
    x = denoise_ref(e["sd"], e["cfg"], R.pack_latents(noise), cond, s["pe"][:1].cpu(), s["pool"][:1].cpu(), 8, 8, N, 3.5)
    _, ref_u8 = V.latents_to_image(s["sd_dec"], s["vcfg"], x, 16, 16)
    rel = _rel_rmse(out[0], x[0])
    prmse = float(((px[0].float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"fill 128x128, {N} steps: latents rel-RMSE {rel:.4f}, pixel RMSE {prmse:.5f}")
    assert out.shape == (1, 64, LAT)
    assert rel < 2e-2 and prmse < 1e-2


def test_control_matches_cpu_loop(setup):
    """128 x 128, 4 steps: eps for the control image first, then the noise."""
    s = setup
    e, n, N = s["ctrl"], 128, 4
    img, u8 = _image(n, 3)
    kw = _fill_kw(s, n, control_image=img)
    out = e["pipe"](generator=_gen(8), output_type="latent", **kw).images
    px = e["pipe"](generator=_gen(8), output_type="np", **kw).images
    g = _gen(8)
    eps = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
    noise = torch.randn((1, 16, 16, 16), generator=g, device="cuda", dtype=BF).cpu()
    mom = encode_ref(s["sd_enc"], s["vcfg"], preprocess_u8(u8))
    cond = latents_ref(mom, eps, None, 0.0, SCALING, SHIFT)
    x = denoise_ref(e["sd"], e["cfg"], R.pack_latents(noise), cond, s["pe"][:1].cpu(), s["pool"][:1].cpu(), 8, 8, N, 3.5)
    _, ref_u8 = V.latents_to_image(s["sd_dec"], s["vcfg"], x, 16, 16)
    rel = _rel_rmse(out[0], x[0])
    prmse = float(((px[0].float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"control 128x128, {N} steps: latents rel-RMSE {rel:.4f}, pixel RMSE {prmse:.5f}")
    assert rel < 2e-2 and prmse < 1e-2


@pytest.mark.parametrize("case", ["fill_default", "fill_latents", "fill_masked_image_latents", "control_default", "control_latents",
                                  "control_image_as_latents"])
def test_generator_position_after_a_call(setup, case):
    """Fill: noise [B] (not with latents=), then eps [B_img] (not with masked_image_latents=).  Control: eps [B_img] (not with a latent
    control_image), then noise [B] (not with latents=).  The generator's next draw after the call is the expected one."""
    s = setup
    img, _ = _image(128, 9)
    shape = (1, 16, 16, 16)
    g, r = _gen(13), _gen(13)
    draws = 2
    if case.startswith("fill"):
        kw = _fill_kw(s, 128, image=img, mask_image=_mask(128, "left"), output_type="latent")
        if case == "fill_latents":
            kw["latents"], draws = torch.zeros(1, 64, LAT, dtype=BF, device="cuda"), 1
        elif case == "fill_masked_image_latents":
            kw.pop("image"), kw.pop("mask_image")
            kw["masked_image_latents"], draws = torch.zeros(1, 64, 320, dtype=BF, device="cuda"), 1
        s["fill"]["pipe"](generator=g, **kw)
    else:
        kw = _fill_kw(s, 128, control_image=img, output_type="latent")
        if case == "control_latents":
            kw["latents"], draws = torch.zeros(1, 64, LAT, dtype=BF, device="cuda"), 1
        elif case == "control_image_as_latents":
            kw["control_image"], draws = torch.zeros(1, 16, 16, 16, dtype=BF, device="cuda"), 1
        s["ctrl"]["pipe"](generator=g, **kw)
    after = torch.randn(64, generator=g, device="cuda", dtype=BF)
    for _ in range(draws):
        torch.randn(shape, generator=r, device="cuda", dtype=BF)
    want = torch.randn(64, generator=r, device="cuda", dtype=BF)
    assert torch.equal(_i16(after), _i16(want))


def test_given_conditions_are_used_as_they_are(setup):
    """masked_image_latents = the condition the pipeline would have built -> the same bits; a latent control_image = packed as it is."""
    s = setup
    img, u8 = _image(128, 10)
    mk = _mask(128, "blob")
    lat = torch.randn(1, 64, LAT, generator=torch.Generator().manual_seed(2)).to(BF).cuda()
    keep = lat.clone()
    kw = _fill_kw(s, 128, latents=lat, output_type="latent")
    a = s["fill"]["pipe"](image=img, mask_image=mk, generator=_gen(3), **kw).images
    eps = torch.randn((1, 16, 16, 16), generator=_gen(3), device="cuda", dtype=BF)      # latents given: eps is the first draw
    mask = torch.from_numpy(np.array(mk)).cuda()
    cond = _ops().flux_fill_condition(s["enc"].encode_moments(u8, mask=mask), eps[0], mask, SCALING, SHIFT, 128, 128)
    b = s["fill"]["pipe"](masked_image_latents=cond[None], **kw).images
    assert torch.equal(_i16(a), _i16(b)) and torch.equal(_i16(lat), _i16(keep))      # the caller's latents are not written
    cl = torch.randn(1, 16, 16, 16, generator=torch.Generator().manual_seed(4)).to(BF).cuda()
    c = s["ctrl"]["pipe"](control_image=cl, **kw).images
    tr = s["ctrl"]["tr"]
    sig = _prepare(tr, s["pe"][0], s["pool"][0], 8, 8, 4)
    tr.set_channel_condition(R.pack_latents(cl)[0].contiguous())
    x = lat[0].clone()
    tr.denoise(x, sig)
    torch.cuda.synchronize()
    assert torch.equal(_i16(c[0]), _i16(x))


def test_images_in_flight_and_condition_per_context(setup):
    """num_images_per_prompt = 3 with 1 and 2 images in flight: the same bits.  Two masks in one call give different images, each equal to
    its single-call run: context k carries sample k's condition and nothing leaks between contexts."""
    s = setup
    p = s["fill"]["pipe"]
    img, _ = _image(128, 11)
    kw = _fill_kw(s, 128, image=img, output_type="latent")
    old = p.images_in_flight
    try:
        runs = {}
        for G in (1, 2):
            p.images_in_flight = G
            runs[G] = p(mask_image=_mask(128, "blob"), num_images_per_prompt=3, generator=_gen(5), **kw).images.clone()
        assert runs[1].shape == (3, 64, LAT) and torch.equal(_i16(runs[1]), _i16(runs[2]))
        assert not torch.equal(_i16(runs[1][0]), _i16(runs[1][1]))
        lat = torch.randn(2, 64, LAT, generator=torch.Generator().manual_seed(6)).to(BF).cuda()
        p.images_in_flight = 2
        both = p(mask_image=[_mask(128, "left"), _mask(128, "top")], num_images_per_prompt=2, latents=lat, generator=_gen(6), **kw).images.clone()
        singles = [p(mask_image=_mask(128, k), latents=lat[b:b + 1], generator=_gen(6), **kw).images[0].clone() for b, k in enumerate(("left", "top"))]
        same_mask = p(mask_image=_mask(128, "left"), latents=lat[1:2], generator=_gen(6), **kw).images[0]
    finally:
        p.images_in_flight = old
    torch.cuda.synchronize()
    assert torch.equal(_i16(both[0]), _i16(singles[0])) and torch.equal(_i16(both[1]), _i16(singles[1]))
    assert not torch.equal(_i16(both[1]), _i16(same_mask))      # sample 1 read the second mask, not the first


def test_pil_output_and_aligner_shaped_prompt(setup):
    s = setup
    fc = s["fill"]["cfg"]
    g = torch.Generator().manual_seed(31)
    pe = torch.randn(1, 128, fc.joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(1, fc.pooled_projection_dim, generator=g).bfloat16().cuda()
    m = torch.zeros(256, 256)
    m[64:192, 64:192] = 1.0
    for pipe, kw in ((s["fill"]["pipe"], dict(image=_image(256, 10)[0], mask_image=m)), (s["ctrl"]["pipe"], dict(control_image=_image(256, 12)[0]))):
        out = pipe(prompt_embeds=pe, pooled_prompt_embeds=pool, height=256, width=256, num_inference_steps=4, guidance_scale=3.5,
                   generator=_gen(1), **kw)
        im = out.images[0]
        assert im.size == (256, 256) and im.mode == "RGB"


# ---- the 8-bit modes on a conditioned engine -------------------------------------------------------------------------------------------
def _eightbit_case(setup):
    e = setup["fill"]
    cfg = e["cfg"]
    h2, w2, T = 12, 20, 65
    lat, cond, pe, pool = _fwd_inputs(cfg, h2, w2, T, seed=77)
    img_ids, txt_ids = R.latent_image_ids(h2, w2), torch.zeros(T, 3)
    t, g = torch.tensor([0.7324]), torch.tensor([3.5])
    ref_args = (e["sd"], cfg, lat, cond, pe, pool, t.bfloat16(), img_ids.bfloat16(), txt_ids.bfloat16(), g)
    run = lambda: e["tr"].forward(torch.cat([lat, cond], dim=2).cuda(), pe.cuda(), pool.cuda(), t.bfloat16().cuda(), img_ids, txt_ids, g)[0].clone()
    return e["tr"], ref_args, run


def test_fp8_mode_on_a_conditioned_engine(setup):
    """test_fp8_mode_matches_fp8_oracle's bars: < 3e-2 against the fp8 oracle, deviation from bf16 < 0.15, back to bf16 bit-exact."""
    m, ref_args, run = _eightbit_case(setup)
    ref16 = forward_ref(*ref_args)
    R.FP8_BLOCK_LINEARS = True
    try:
        ref8 = forward_ref(*ref_args)
    finally:
        R.FP8_BLOCK_LINEARS = False
    out16 = run()
    try:
        m.set_precision("fp8")
        out8 = run()
    finally:
        m.set_precision("bf16")
    back = run()
    torch.cuda.synchronize()
    e88, e816, o816 = _rel_rmse(out8, ref8), _rel_rmse(out8, out16), _rel_rmse(ref8, ref16)
    print(f"Cin 384: hip-fp8~oracle-fp8 {e88:.4f}   hip-fp8~hip-bf16 {e816:.4f}   oracle-fp8~oracle-bf16 {o816:.4f}")
    assert e88 < 3e-2
    assert 0 < e816 < 0.15
    assert torch.equal(back, out16)


def test_int8_mode_on_a_conditioned_engine(setup):
    """test_int8_mode_matches_int8_oracle's bars."""
    m, ref_args, run = _eightbit_case(setup)
    ref16 = forward_ref(*ref_args)
    R.INT8_BLOCK_LINEARS = True
    try:
        ref8 = forward_ref(*ref_args)
    finally:
        R.INT8_BLOCK_LINEARS = False
    out16 = run()
    try:
        m.set_precision("int8")
        out8 = run()
    finally:
        m.set_precision("bf16")
    torch.cuda.synchronize()
    e16, e88, d_hip, d_ref = _rel_rmse(out16, ref16), _rel_rmse(out8, ref8), _rel_rmse(out8, out16), _rel_rmse(ref8, ref16)
    print(f"Cin 384: hip~bf16-oracle {e16:.4f}  hip-int8~oracle-int8 {e88:.4f}  int8~bf16 hip {d_hip:.4f} oracle {d_ref:.4f}")
    assert e16 < 2e-2 and e88 < 2e-2
    assert d_hip < 3e-2 and abs(d_hip - d_ref) < 0.5 * d_ref + 2e-3


def test_int8_smoothing_history_fp8_attention_on_a_conditioned_engine(setup):
    """int8 + smoothing + fp8 attention with dynamic and with history scales over a 4-step denoise: finite, history tracking the dynamic
    path by test_int8_history_scales_track_the_dynamic_path's inequality, repeatable bit for bit, and a new image's channel condition does
    not meet the previous image's per-token history (the second image alone equals the second image after the first)."""
    e = setup["fill"]
    m, cfg = e["tr"], e["cfg"]
    h2 = w2 = 16
    T, n = 40, 4
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(h2 * w2, LAT, generator=g).bfloat16().cuda()
    conds = [torch.randn(h2 * w2, 320, generator=g).bfloat16().cuda() for _ in range(2)]
    pe = torch.randn(T, cfg.joint_attention_dim, generator=g).bfloat16().cuda()
    pool = torch.randn(cfg.pooled_projection_dim, generator=g).bfloat16().cuda()
    sig = _prepare(m, pe, pool, h2, w2, n)

    def run(cond):
        m.set_channel_condition(cond)
        x = lat.clone()
        m.denoise(x, sig)
        torch.cuda.synchronize()
        return x.float().cpu()

    outs = {}
    try:
        outs["bf16"] = run(conds[0])
        m.set_attention("fp8")
        for name, kw in (("dynamic", dict(precision="int8", smoothing=True)), ("history", dict(precision="int8", smoothing=True, act_scales="history")),
                         ("history2", dict(precision="int8", smoothing=True, act_scales="history"))):
            m.set_precision(**kw)
            outs[name] = run(conds[0])
        second_after_first = run(conds[1])
        m.set_precision("int8", smoothing=True, act_scales="history")      # forgets the calibration and the history: a fresh start
        run(conds[1])                                                      # (the calibration forward is part of a first run)
        outs["first"] = run(conds[0])
        second_after_first2 = run(conds[1])
    finally:
        m.set_attention("bf16")
        m.set_precision("bf16")
    rel = lambda a, b: float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    d_int8, d_hist, d_hd = rel(outs["dynamic"], outs["bf16"]), rel(outs["history"], outs["bf16"]), rel(outs["history"], outs["dynamic"])
    print(f"Cin 384, 4-step denoise, int8 + smoothing + fp8 attention: dynamic~bf16 {d_int8:.4f}  history~bf16 {d_hist:.4f}  history~dynamic {d_hd:.4f}")
    assert all(torch.isfinite(v).all() for v in outs.values())
    assert torch.equal(outs["history"], outs["history2"])
    assert 0 < d_hd and d_hist < 1.5 * d_int8 + 1e-3
    assert not torch.equal(second_after_first, outs["history"])
    assert torch.equal(second_after_first, second_after_first2)
