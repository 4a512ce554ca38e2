"""GPU parity of the VAE encoder path (td_conv3x3_s2_nhwc_bf16, td_vae_image_to_nhwc_bf16, td_vae_latents_from_moments, td_vae_encode)
against the test-local CPU restatement (tests/vae_encoder_common.py, built on oracle/vae_ref.py).

Tolerances: the stride-2 conv <= 2^-6 of the output scale (as test_conv3x3_implicit_gemm); the two boundary kernels bit-exact with
the bf16 torch statements (the sampled posterior within one bf16 ulp: exp may differ in the last fp32 bit); the encoder end to end
rel-RMSE < 3e-2 of the moments (as the decoder's end-to-end bar)."""
import json
import os
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import vae_ref as V
from vae_encoder_common import encode_ref, encoder_init_weights, latents_ref, nhwc_moments_to_nchw, preprocess_u8

pytestmark = pytest.mark.gpu


def _ops():
    from thinkdiff.ops import register
    return register()      # torch.ops.thinkdiff_hip (loads the op library)


def _nhwc(t):
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()


def _rel_rmse(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


@pytest.mark.parametrize("Hin,Win,Cin,Cout", [(16, 16, 64, 64), (32, 48, 128, 128), (64, 64, 256, 256), (18, 22, 64, 8)])
def test_conv3x3_stride2(hip, Hin, Win, Cin, Cout):
    """Downsample2D(use_conv, padding=0).  (64, 64, 256, 256): with the output extent as the A descriptor's range every row below
    the first quarter of the input would read as zero.
    One number against the output scale; the per-element bounds and the edge shapes are in tests/test_vae_conv_fp64_gpu.py."""
    g = torch.Generator().manual_seed(Hin * Win + Cin)
    x = torch.randn(1, Cin, Hin, Win, generator=g).bfloat16()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).bfloat16()
    b = torch.randn(Cout, generator=g).bfloat16()
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), b.float(), stride=2).bfloat16()
    y = hip.conv3x3_s2_nhwc(_nhwc(x).cuda(), hip.conv3x3_pack_weight(w.cuda()), b.cuda(), Hin, Win, Cout)
    torch.cuda.synchronize()
    assert y.shape == ((Hin // 2) * (Win // 2), Cout)
    got, want = y.float().cpu(), _nhwc(ref).float()
    assert torch.isfinite(got).all()
    err = (got - want).abs().max() / want.abs().max()
    assert err < 2.0 ** -6, f"rel-to-scale err {err:.3e}"
    # the bottom rows and the right column (the padded taps) are right too
    lower = (got.view(Hin // 2, Win // 2, Cout)[Hin // 4:] - want.view(Hin // 2, Win // 2, Cout)[Hin // 4:]).abs().max() / want.abs().max()
    assert lower < 2.0 ** -6


def test_image_in_bit_exact(hip):
    H, W = 32, 48
    g = torch.Generator().manual_seed(4)
    u8 = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)          # every code value
    got = hip.vae_image_to_nhwc(u8.cuda(), 64)
    f = torch.rand(3, H, W, generator=g)
    f.view(-1)[:4] = torch.tensor([0.0, 1.0, 0.5, 1.0 / 3.0])
    gotf = hip.vae_image_to_nhwc(f.cuda(), 64)
    torch.cuda.synchronize()
    want = _nhwc(preprocess_u8(u8))
    assert torch.equal(got[:, :3].cpu().view(torch.int16), want.view(torch.int16))
    wantf = _nhwc((2 * f - 1)[None].bfloat16())
    assert torch.equal(gotf[:, :3].cpu().view(torch.int16), wantf.view(torch.int16))
    assert not got[:, 3:].cpu().view(torch.int16).any() and not gotf[:, 3:].cpu().view(torch.int16).any()


def _moments(h, w, C=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(1, C, h, w, generator=g) * 1.5
    logvar = torch.rand(1, C, h, w, generator=g) * 60 - 40          # [-40, 20): the clamp at -30 is taken
    logvar.view(-1)[:8] = torch.tensor([25.0, 20.5, -30.5, 19.9, -29.0, 0.0, -0.5, 3.0])
    return torch.cat([mean, logvar], 1).bfloat16()


@pytest.mark.parametrize("sigma", [None, 1.0, 0.5, 0.0123])
def test_latents_from_moments_mode_bit_exact(hip, sigma):
    h, w = 16, 24
    mom = _moments(h, w, seed=1)
    noise = torch.randn(1, 16, h, w, generator=torch.Generator().manual_seed(2)).bfloat16()
    nz = None if sigma is None else noise
    want = latents_ref(mom, None, nz, sigma or 0.0, 0.3611, 0.1159)[0]
    got = _ops().vae_latents_from_moments(_nhwc(mom).cuda(), None, None if nz is None else nz[0].cuda().contiguous(),
                                                           float(sigma or 0.0), 0.3611, 0.1159, h, w)
    torch.cuda.synchronize()
    assert got.shape == want.shape == ((h // 2) * (w // 2), 64)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("sigma", [None, 0.5])
def test_latents_from_moments_sample_within_one_ulp(hip, sigma):
    h, w = 16, 24
    mom = _moments(h, w, seed=3)
    g = torch.Generator().manual_seed(5)
    eps = torch.randn(1, 16, h, w, generator=g).bfloat16()
    noise = torch.randn(1, 16, h, w, generator=g).bfloat16() if sigma is not None else None
    want = latents_ref(mom, eps, noise, sigma or 0.0, 0.3611, 0.1159)[0].float()
    got = _ops().vae_latents_from_moments(_nhwc(mom).cuda(), eps[0].cuda().contiguous(),
                                                           None if noise is None else noise[0].cuda().contiguous(),
                                                           float(sigma or 0.0), 0.3611, 0.1159, h, w).float().cpu()
    # one bf16 ulp of the largest term that went into the element (std * eps may exceed the result after the mean cancels it)
    _, logvar = torch.chunk(mom.float(), 2, dim=1)
    term = latents_ref(torch.cat([torch.zeros_like(mom[:, :16]), mom[:, 16:]], 1), eps.abs(), None, 0.0, 0.3611, 0.0)[0].float().abs()
    bound = 2.0 ** -7 * torch.maximum(want.abs(), term) + 1e-30
    assert ((got - want).abs() <= bound).all(), float(((got - want).abs() / bound).max())
    assert (got == want).float().mean() > 0.99


def _encoder(cfg, seed, max_size):
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLEncoder
    sd = encoder_init_weights(cfg, seed=seed)
    m = AutoencoderKLEncoder(AutoencoderKLConfig(block_out_channels=cfg.block_out_channels), max_image_size=max_size)
    m.load_state_dict(sd)
    return sd, m


def test_tiny_encoder_matches_restatement(hip):
    cfg = V.tiny_config()
    sd, m = _encoder(cfg, seed=7, max_size=(64, 64))
    H, W = 32, 48
    u8 = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    ref = encode_ref(sd, cfg, preprocess_u8(u8))
    got = m.encode_moments(u8.cuda())
    torch.cuda.synchronize()
    assert got.shape == (H // 2 * W // 2, 32)
    rel = _rel_rmse(nhwc_moments_to_nchw(got.cpu(), H // 2, W // 2), ref)
    print(f"tiny encoder {H}x{W}: moments rel-RMSE {rel:.4f}")
    assert rel < 3e-2
    # the float [0, 1] CHW source goes through the same arithmetic
    gotf = m.encode_moments((u8.permute(2, 0, 1).float() / 255).cuda())
    rel_f = _rel_rmse(nhwc_moments_to_nchw(gotf.cpu(), H // 2, W // 2), ref)
    assert rel_f < 3e-2


@pytest.mark.parametrize("n", [256, 512])
def test_full_architecture_encoder_matches_restatement(hip, n):
    """The FLUX.1 VAE encoder at full width (128/256/512/512, 2 layers per block, 512-wide single-head mid attention)."""
    cfg = V.VaeConfig()
    sd, m = _encoder(cfg, seed=11, max_size=(n, n))
    u8 = torch.randint(0, 256, (n, n, 3), generator=torch.Generator().manual_seed(n), dtype=torch.uint8)
    t0 = time.time()
    ref = encode_ref(sd, cfg, preprocess_u8(u8))
    t_cpu = time.time() - t0
    got = m.encode_moments(u8.cuda())
    torch.cuda.synchronize()
    rel = _rel_rmse(nhwc_moments_to_nchw(got.cpu(), n // 8, n // 8), ref)
    print(f"full-architecture encoder {n}x{n}: moments rel-RMSE {rel:.4f} (CPU leg {t_cpu:.1f} s)")
    assert got.shape == ((n // 8) ** 2, 32) and rel < 3e-2


def test_full_size_encoder_1024_deterministic(hip):
    from thinkdiff.models.flux_vae import AutoencoderKLEncoder
    m = AutoencoderKLEncoder(max_image_size=(1024, 1024)).init_random(seed=2)
    u8 = torch.randint(0, 256, (1024, 1024, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    a = m.encode_moments(u8)
    b = m.encode_moments(u8)
    torch.cuda.synchronize()
    assert a.shape == (128 * 128, 32) and torch.isfinite(a.float()).all() and a.float().abs().max() > 0
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    # the torch op is the same computation
    c = _ops().vae_encode_moments(int(m._h.value), u8, 1024, 1024)
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))


def _write_vae_dir(root, cfg, sd):
    from safetensors.torch import save_file
    os.makedirs(os.path.join(root, "vae"))
    with open(os.path.join(root, "vae", "config.json"), "w") as fh:
        json.dump({"_class_name": "AutoencoderKL", "in_channels": 3, "out_channels": 3, "latent_channels": cfg.latent_channels,
                   "block_out_channels": list(cfg.block_out_channels), "layers_per_block": cfg.layers_per_block,
                   "norm_num_groups": cfg.norm_groups, "scaling_factor": 0.3611, "shift_factor": 0.1159,
                   "use_quant_conv": False, "use_post_quant_conv": False, "mid_block_add_attention": True}, fh)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(root, "vae", "diffusion_pytorch_model.safetensors"))


def test_loader_and_refusals(hip, tmp_path):
    from thinkdiff import _hip
    from thinkdiff.models.flux_vae import AutoencoderKL, AutoencoderKLConfig, AutoencoderKLDecoder, AutoencoderKLEncoder
    cfg = V.tiny_config()
    sd_enc, sd_dec = encoder_init_weights(cfg, seed=5), V.init_weights(cfg, seed=6)
    _write_vae_dir(str(tmp_path / "full"), cfg, {**sd_enc, **sd_dec})
    vae = AutoencoderKL.from_pretrained(str(tmp_path / "full"), max_latent_size=(16, 16), max_image_size=(64, 64))
    H, W = 32, 32
    u8 = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    got = vae.encoder.encode_moments(u8.cuda())
    ref = encode_ref(sd_enc, cfg, preprocess_u8(u8))
    assert _rel_rmse(nhwc_moments_to_nchw(got.cpu(), H // 2, W // 2), ref) < 3e-2
    # encode(x).latent_dist as in diffusers: NCHW mean / logvar, mode() = mean
    dist = vae.encode((u8.permute(2, 0, 1).float() / 255)[None].cuda()).latent_dist
    assert dist.mean.shape == (1, 16, H // 2, W // 2) and dist.logvar.shape == dist.mean.shape and dist.std.shape == dist.mean.shape
    assert torch.equal(dist.mode().view(torch.int16), dist.mean.view(torch.int16))
    s = dist.sample(torch.Generator(device="cuda").manual_seed(0))
    assert s.shape == dist.mean.shape and torch.isfinite(s.float()).all()
    packed = (torch.randn(1, (H // 4) * (W // 4), 64, generator=torch.Generator().manual_seed(3)) * 0.8).bfloat16()
    ref_img, _ = V.latents_to_image(sd_dec, cfg, packed, H // 2, W // 2)
    img = vae.decode_packed(packed[0].cuda(), H // 2, W // 2, output_type="pt")
    assert _rel_rmse(img, ref_img[0]) < 3e-2
    # a checkpoint without one encoder tensor is refused
    _write_vae_dir(str(tmp_path / "partial"), cfg, {**{k: v for k, v in sd_enc.items() if k != "encoder.conv_out.bias"}, **sd_dec})
    with pytest.raises(KeyError, match="encoder"):
        AutoencoderKLEncoder.from_pretrained(str(tmp_path / "partial"), max_image_size=(64, 64))
    # size refusals come back as errors, before any launch
    enc = vae.encoder
    for hh, ww in [(24, 32), (32, 40), (80, 80), (64, 96)]:
        with pytest.raises(_hip.ThinkDiffHipError):
            enc.encode_moments(torch.zeros(hh, ww, 3, dtype=torch.uint8, device="cuda"))
    # the decoder's parameter table is the decoder's alone
    dec = AutoencoderKLDecoder(AutoencoderKLConfig(block_out_channels=cfg.block_out_channels), max_latent_size=(16, 16))
    assert hip.lib().td_vae_num_params(dec._h) == len(V.param_shapes(cfg)) and set(dec.param_table()) == set(V.param_shapes(cfg))
    assert set(enc.param_table()) == set(sd_enc)
