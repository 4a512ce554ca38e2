"""Test-local CPU restatement of the channel-conditioned FLUX pipelines (FLUX.1 Fill, FLUX.1 Canny / Depth), shared by
test_fill_cpu.py and test_flux_fill_gpu.py.

**Parity unpinned**: restated from the published diffusers >= 0.32 sources (`pipeline_flux_fill.py` `prepare_mask_latents` /
`__call__`, `pipeline_flux_control.py` `prepare_image` / `__call__`), on top of oracle/flux_ref.py and vae_encoder_common.py; the
spec is the docstrings of thinkdiff/models/flux_fill.py and flux_control.py.  Every statement runs on bf16 tensors, as the
pipelines do.

The transformer oracle sizes `proj_out` by `in_channels`; a channel-conditioned checkpoint writes 64 columns.  `conditioned_weights`
therefore builds the oracle's state dict for in_channels = Cin and hands the engine `proj_out.weight[:64]` / `.bias[:64]` (everything
else as it is); `forward_ref` takes the first 64 output columns of the oracle.  `proj_out` is the oracle's last statement and the
output columns of a Linear are independent, so the slice is exact."""
import torch

from oracle import flux_ref as R
from vae_encoder_common import latents_ref

LAT = 64      # packed latent channels (4 x 16)


def binarize(mask: torch.Tensor) -> torch.Tensor:
    """mask_processor's binarization: uint8 [H, W] -> float32(u8) / 255 >= 0.5 (u8 >= 128); float [H, W] -> v >= 0.5; float32 0 / 1."""
    m = mask.float() / 255 if mask.dtype == torch.uint8 else mask.float().clone()
    return (m >= 0.5).float()


def unshuffle_ref(mask: torch.Tensor) -> torch.Tensor:
    """prepare_mask_latents on one mask [H, W]: binarize, view(h, 8, w, 8).permute(1, 3, 0, 2).reshape(64, h, w), _pack_latents ->
    bf16 [S, 256] of 0 / 1."""
    m = binarize(mask)
    H, W = m.shape
    h, w = H // 8, W // 8
    m = m.view(h, 8, w, 8).permute(1, 3, 0, 2).reshape(1, 64, h, w)
    return R.pack_latents(m.to(torch.bfloat16))[0]


def unshuffle_source(H: int, W: int):
    """The closed form: (rows, cols) int64 [S, 256] with out[tok, (py*8 + px)*4 + dy*2 + dx] = m[8(2Y + dy) + py, 8(2X + dx) + px],
    tok = Y (W/16) + X."""
    S = (H // 16) * (W // 16)
    tok = torch.arange(S)[:, None]
    col = torch.arange(256)[None, :]
    Y, X = tok // (W // 16), tok % (W // 16)
    q, dy, dx = col // 4, (col // 2) % 2, col % 2
    py, px = q // 8, q % 8
    return 8 * (2 * Y + dy) + py, 8 * (2 * X + dx) + px


def masked_image_ref(x_pre: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """masked_image = image * (1 - mask) on the preprocessed fp32 image [1, 3, H, W], then .to(bf16)."""
    return (x_pre.float() * (1 - binarize(mask))[None, None]).to(torch.bfloat16)


def preprocess_f32(u8_hwc: torch.Tensor) -> torch.Tensor:
    """VaeImageProcessor.preprocess(PIL) in fp32: uint8 [H, W, 3] -> [1, 3, H, W] in [-1, 1]."""
    return (2 * (u8_hwc.float() / 255) - 1).permute(2, 0, 1)[None].contiguous()


def fill_condition_ref(moments_nchw: torch.Tensor, eps, mask: torch.Tensor, scaling: float, shift: float) -> torch.Tensor:
    """[S, 320]: packed (sample(moments, eps) - shift) * scaling | the unshuffled mask.  moments bf16 [1, 32, h, w], eps [1, 16, h, w] or None."""
    return torch.cat([latents_ref(moments_nchw, eps, None, 0.0, scaling, shift)[0], unshuffle_ref(mask)], dim=-1)


def conditioned_weights(c_in: int, seed: int, num_layers: int = 1, num_single_layers: int = 1):
    """(oracle config, oracle state dict, engine state dict) of a tiny transformer with in_channels = c_in, out_channels = 64."""
    cfg = R.tiny_config(in_channels=c_in, num_layers=num_layers, num_single_layers=num_single_layers)
    sd = R.init_weights(cfg, seed=seed)
    eng = dict(sd)
    eng["proj_out.weight"] = sd["proj_out.weight"][:LAT].contiguous()
    eng["proj_out.bias"] = sd["proj_out.bias"][:LAT].contiguous()
    return cfg, sd, eng


def build_engine(cfg, sd_engine, out_channels=LAT, **caps):
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig
    caps = {**dict(max_img_tokens=256, max_txt_tokens=128, max_steps=8), **caps}
    m = FluxTransformer2DModel(FluxTransformerConfig(
        in_channels=cfg.in_channels, out_channels=out_channels, num_layers=cfg.num_layers, num_single_layers=cfg.num_single_layers,
        num_attention_heads=cfg.num_attention_heads, joint_attention_dim=cfg.joint_attention_dim,
        pooled_projection_dim=cfg.pooled_projection_dim, guidance_embeds=cfg.guidance_embeds), **caps)
    m.load_state_dict(sd_engine)
    return m


def forward_ref(sd, cfg, lat, cond, pe, pool, t, img_ids, txt_ids, guidance):
    """The oracle on torch.cat([latents, cond], dim=2), first 64 output columns."""
    return R.transformer_forward(sd, cfg, torch.cat([lat, cond.to(lat.dtype)], dim=2), pe, pool, t, img_ids, txt_ids, guidance)[..., :LAT]


def denoise_ref(sd, cfg, lat, cond, pe, pool, h2, w2, n, guidance_scale):
    """FluxFillPipeline / FluxControlPipeline's loop on packed latents [1, S, 64] with the condition [1, S, Cc] concatenated in front of
    every transformer call; the scheduler step as oracle.flux_ref.denoise states it.  The full schedule from pure noise."""
    dt = lat.dtype
    sig = R.make_sigmas(n, lat.shape[1])
    timesteps = torch.from_numpy(sig[:-1]) * 1000.0
    img_ids = R.latent_image_ids(h2, w2).to(dt)
    txt_ids = torch.zeros(pe.shape[1], 3).to(dt)
    guidance = torch.full([1], guidance_scale, dtype=torch.float32) if cfg.guidance_embeds else None
    sig_t = torch.from_numpy(sig)
    x = lat
    for i in range(n):
        t = timesteps[i].expand(1).to(dt)
        v = forward_ref(sd, cfg, x, cond, pe, pool, t / 1000, img_ids, txt_ids, guidance)
        x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
    return x
