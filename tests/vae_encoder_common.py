"""Test-local CPU restatement of the FLUX VAE encoder side (shared by test_vae_encoder_gpu.py and test_flux_img2img_gpu.py).

**Parity unpinned**, like oracle/vae_ref.py: restated from the published diffusers 0.31.0 sources ([ext] models/autoencoders/vae.py
`Encoder`, unet_2d_blocks.py `DownEncoderBlock2D` / `UNetMidBlock2D`, downsampling.py `Downsample2D` (use_conv, padding=0:
F.pad(x, (0,1,0,1)) + stride-2 conv), vae.py `DiagonalGaussianDistribution`, image_processor.py `VaeImageProcessor.preprocess`,
pipeline_flux_img2img.py `_encode_vae_image` / `prepare_latents`, scheduling_flow_match_euler_discrete.py `scale_noise`), built on
oracle/vae_ref.py's `_gn`, `_resnet` and `_mid_attention`.  Every statement runs on bf16 tensors, as the pipeline does."""
from typing import Dict

import torch
import torch.nn.functional as F

from oracle import flux_ref as R
from oracle import vae_ref as V


def encoder_param_shapes(cfg: V.VaeConfig) -> Dict[str, tuple]:
    s: Dict[str, tuple] = {}
    chans = list(cfg.block_out_channels)
    s["encoder.conv_in.weight"] = (chans[0], cfg.out_channels, 3, 3); s["encoder.conv_in.bias"] = (chans[0],)
    prev = chans[0]
    for b, co in enumerate(chans):
        for r in range(cfg.layers_per_block):
            V._resnet_shapes(s, f"encoder.down_blocks.{b}.resnets.{r}.", prev if r == 0 else co, co)
        if b != len(chans) - 1:
            s[f"encoder.down_blocks.{b}.downsamplers.0.conv.weight"] = (co, co, 3, 3)
            s[f"encoder.down_blocks.{b}.downsamplers.0.conv.bias"] = (co,)
        prev = co
    cmid = chans[-1]
    V._resnet_shapes(s, "encoder.mid_block.resnets.0.", cmid, cmid)
    V._resnet_shapes(s, "encoder.mid_block.resnets.1.", cmid, cmid)
    a = "encoder.mid_block.attentions.0."
    s[a + "group_norm.weight"] = (cmid,); s[a + "group_norm.bias"] = (cmid,)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        s[a + n + ".weight"] = (cmid, cmid); s[a + n + ".bias"] = (cmid,)
    s["encoder.conv_norm_out.weight"] = (cmid,); s["encoder.conv_norm_out.bias"] = (cmid,)
    s["encoder.conv_out.weight"] = (2 * cfg.latent_channels, cmid, 3, 3); s["encoder.conv_out.bias"] = (2 * cfg.latent_channels,)
    return s


def encoder_init_weights(cfg: V.VaeConfig, seed: int = 0, dtype=torch.bfloat16):
    """oracle/vae_ref.init_weights' scheme (1 / sqrt(fan_in) weights) on the encoder's tensors."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in encoder_param_shapes(cfg).items():
        if "norm" in k and k.endswith("weight"):
            sd[k] = (1.0 + 0.05 * torch.randn(shp, generator=g)).to(dtype)
        elif len(shp) == 4:
            sd[k] = (torch.randn(shp, generator=g) / (shp[1] * shp[2] * shp[3]) ** 0.5).to(dtype)
        elif len(shp) == 2:
            sd[k] = (torch.randn(shp, generator=g) / shp[1] ** 0.5).to(dtype)
        else:
            sd[k] = (0.02 * torch.randn(shp, generator=g)).to(dtype)
    return sd


def preprocess_u8(u8_hwc: torch.Tensor) -> torch.Tensor:
    """VaeImageProcessor.preprocess(PIL) + .to(bf16): uint8 [H, W, 3] -> bf16 [1, 3, H, W] in [-1, 1]."""
    x = u8_hwc.float() / 255
    x = 2 * x - 1
    return x.permute(2, 0, 1)[None].contiguous().bfloat16()


def encode_ref(sd, cfg: V.VaeConfig, x: torch.Tensor) -> torch.Tensor:
    """Encoder(x) with double_z, no quant_conv: x bf16 [B, 3, H, W] in [-1, 1] -> moments [B, 2C, H/f, W/f] (mean | logvar)."""
    g = cfg.norm_groups
    nb = len(cfg.block_out_channels)
    h = F.conv2d(x, sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"], padding=1)
    for b in range(nb):
        for r in range(cfg.layers_per_block):
            h = V._resnet(sd, f"encoder.down_blocks.{b}.resnets.{r}.", h, g)
        if b != nb - 1:
            p = f"encoder.down_blocks.{b}.downsamplers.0.conv."
            h = F.conv2d(F.pad(h, (0, 1, 0, 1)), sd[p + "weight"], sd[p + "bias"], stride=2)
    h = V._resnet(sd, "encoder.mid_block.resnets.0.", h, g)
    h = V._mid_attention(sd, "encoder.mid_block.attentions.0.", h, g)
    h = V._resnet(sd, "encoder.mid_block.resnets.1.", h, g)
    h = F.silu(V._gn(sd, "encoder.conv_norm_out", h, g))
    return F.conv2d(h, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"], padding=1)


def latents_ref(moments: torch.Tensor, eps, noise, sigma, scaling: float, shift: float) -> torch.Tensor:
    """moments bf16 [B, 2C, h, w] -> packed start latents [B, (h/2)(w/2), 4C]: DiagonalGaussianDistribution(.sample(eps) or .mode()),
    _encode_vae_image's (z - shift) * scaling, scale_noise with sigma = sigmas.to(bf16) (noise None: skipped), _pack_latents."""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    z = mean if eps is None else mean + std * eps
    z = (z - shift) * scaling
    if noise is not None:
        sig = torch.tensor([sigma], dtype=torch.float32).to(z.dtype)
        while sig.dim() < z.dim():
            sig = sig.unsqueeze(-1)
        z = sig * noise + (1.0 - sig) * z
    return R.pack_latents(z)


def nhwc_moments_to_nchw(m: torch.Tensor, h: int, w: int) -> torch.Tensor:
    return m.view(h, w, -1).permute(2, 0, 1)[None].contiguous()
