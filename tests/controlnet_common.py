"""Test-local CPU restatement of the FLUX ControlNet, shared by test_controlnet_cpu.py and test_flux_controlnet_gpu.py.

**Parity unpinned**: restated from the published diffusers sources (`controlnet_flux.py` FluxControlNetModel.forward,
`transformer_flux.py` FluxTransformer2DModel.forward with `controlnet_block_samples` / `controlnet_single_block_samples`,
`pipeline_flux_controlnet.py` __call__), composed from oracle/flux_ref.py; the spec is the docstring of
thinkdiff/models/flux_controlnet.py.  Every statement runs on tensors of the dtype it is given (bf16 as the pipeline does, fp32 for the
error yardstick).

Weights: `R.init_weights` for the part a ControlNet shares with the transformer; its own Linears are drawn with std 0.02
(`controlnet_x_embedder`, the mode embedding) and **std 0.005** (the output Linears `controlnet_blocks.*`, `controlnet_single_blocks.*`).
At std 0.005 the residuals move the tiny main model's output by 0.16 - 0.32 rel-RMSE and another control image by 0.15 - 0.31 -- far
above the 2e-2 parity bar -- while the reference's own bf16-vs-fp32 distance stays the plain model's (0.035 vs 0.036); at std 0.02 the
residuals swamp the output, which would hide errors of the main path."""
import math

import torch
import torch.nn.functional as F

from oracle import flux_ref as R

LAT = 64
BF = torch.bfloat16


def rel_rmse(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def main_config():
    return R.tiny_config(num_layers=2, num_single_layers=3)


def cn_config(n_d, n_s):
    return R.tiny_config(num_layers=n_d, num_single_layers=n_s, guidance_embeds=False)


def cn_init_weights(cfg, num_mode=0, seed=0, out_std=0.005, dtype=BF):
    """Seeded synthetic ControlNet checkpoint under the diffusers names."""
    sd = {k: v for k, v in R.init_weights(cfg, seed=seed, dtype=dtype).items() if not k.startswith(("norm_out.", "proj_out."))}
    g = torch.Generator().manual_seed(seed + 1000)
    D = cfg.inner_dim

    def lin(name, out_f, in_f, std):
        sd[name + ".weight"] = (std * torch.randn(out_f, in_f, generator=g)).to(dtype)
        sd[name + ".bias"] = (std * torch.randn(out_f, generator=g)).to(dtype)

    lin("controlnet_x_embedder", D, cfg.in_channels, 0.02)
    for i in range(cfg.num_layers):
        lin(f"controlnet_blocks.{i}", D, D, out_std)
    for i in range(cfg.num_single_layers):
        lin(f"controlnet_single_blocks.{i}", D, D, out_std)
    if num_mode:
        sd["controlnet_mode_embedder.weight"] = (0.02 * torch.randn(num_mode, D, generator=g)).to(dtype)
    return sd


def zero_outputs(sd):
    """The published `zero_module` init of the output Linears."""
    return {k: (torch.zeros_like(v) if k.startswith(("controlnet_blocks.", "controlnet_single_blocks.")) else v) for k, v in sd.items()}


def sample_index(i, n_blocks, n_samples):
    """[ext] transformer_flux.py: interval_control = ceil(len(blocks) / len(samples)); index = i // interval_control."""
    return i // int(math.ceil(n_blocks / n_samples))


def keep_schedule(n, start, end):
    """[ext] pipeline_flux_controlnet.py controlnet_keep."""
    return [1.0 - float(i / n < start or (i + 1) / n > end) for i in range(n)]


def controlnet_forward_ref(sd, cfg, hidden, cond, mode, enc, pooled, timestep, img_ids, txt_ids, guidance, conditioning_scale=None):
    """FluxControlNetModel.forward -> (block_samples, single_samples), each [B, S_img, D]; conditioning_scale None: unscaled.
    hidden / cond [B, S_img, 64]; mode None or an int (union models: `controlnet_mode_embedder.weight` is in sd)."""
    dt = hidden.dtype
    h = R._lin(sd, "x_embedder", hidden) + R._lin(sd, "controlnet_x_embedder", cond)
    timestep = timestep.to(dt) * 1000
    guidance = guidance.to(dt) * 1000 if (guidance is not None and cfg.guidance_embeds) else None
    temb = R.time_text_embed(sd, cfg, timestep, guidance, pooled)
    enc = R._lin(sd, "context_embedder", enc)
    if "controlnet_mode_embedder.weight" in sd:
        if mode is None:
            raise ValueError("`controlnet_mode` cannot be `None` when applying ControlNet-Union")
        emb = sd["controlnet_mode_embedder.weight"][int(mode)][None, None].expand(enc.shape[0], 1, -1)
        enc = torch.cat([emb, enc], dim=1)
        txt_ids = torch.cat([txt_ids[:1], txt_ids], dim=0)
    cos, sin = R.rope_tables(torch.cat([txt_ids, img_ids], dim=0), cfg.axes_dims_rope)
    block_samples, single_samples = [], []
    for i in range(cfg.num_layers):
        enc, h = R.double_block(sd, cfg, i, h, enc, temb, cos, sin)
        block_samples.append(h)
    T = enc.shape[1]
    h = torch.cat([enc, h], dim=1)
    for i in range(cfg.num_single_layers):
        h = R.single_block(sd, cfg, i, h, temb, cos, sin)
        single_samples.append(h[:, T:])
    block_samples = [R._lin(sd, f"controlnet_blocks.{i}", s) for i, s in enumerate(block_samples)]
    single_samples = [R._lin(sd, f"controlnet_single_blocks.{i}", s) for i, s in enumerate(single_samples)]
    if conditioning_scale is not None:
        block_samples = [s * conditioning_scale for s in block_samples]
        single_samples = [s * conditioning_scale for s in single_samples]
    return block_samples, single_samples


def transformer_forward_ref(sd, cfg, hidden, enc, pooled, timestep, img_ids, txt_ids, guidance, block_samples=None, single_samples=None):
    """FluxTransformer2DModel.forward with controlnet_block_samples / controlnet_single_block_samples (None or empty: the plain model)."""
    dt = hidden.dtype
    hidden = R._lin(sd, "x_embedder", hidden)
    timestep = timestep.to(dt) * 1000
    guidance = guidance.to(dt) * 1000 if guidance is not None else None
    temb = R.time_text_embed(sd, cfg, timestep, guidance, pooled)
    enc = R._lin(sd, "context_embedder", enc)
    cos, sin = R.rope_tables(torch.cat([txt_ids, img_ids], dim=0), cfg.axes_dims_rope)
    for i in range(cfg.num_layers):
        enc, hidden = R.double_block(sd, cfg, i, hidden, enc, temb, cos, sin)
        if block_samples:
            hidden = hidden + block_samples[sample_index(i, cfg.num_layers, len(block_samples))]
    T = enc.shape[1]
    hidden = torch.cat([enc, hidden], dim=1)
    for i in range(cfg.num_single_layers):
        hidden = R.single_block(sd, cfg, i, hidden, temb, cos, sin)
        if single_samples:
            hidden = torch.cat([hidden[:, :T], hidden[:, T:] + single_samples[sample_index(i, cfg.num_single_layers, len(single_samples))]], dim=1)
    hidden = hidden[:, T:]
    scale, shift = R._lin(sd, "norm_out.linear", F.silu(temb).to(dt)).chunk(2, dim=1)
    hidden = R._ln(hidden) * (1 + scale)[:, None, :] + shift[:, None, :]
    return R._lin(sd, "proj_out", hidden)


def _bf16_side(fn):
    """The side network runs in bf16 whatever 8-bit mode the reference's block Linears are in (its blocks carry the transformer's names)."""
    saved = R.FP8_BLOCK_LINEARS, R.INT8_BLOCK_LINEARS
    R.FP8_BLOCK_LINEARS = R.INT8_BLOCK_LINEARS = False
    try:
        return fn()
    finally:
        R.FP8_BLOCK_LINEARS, R.INT8_BLOCK_LINEARS = saved


def controlled_forward_ref(sd, cfg, sd_cn, cfg_cn, lat, cond, mode, pe, pool, t, img_ids, txt_ids, guidance, scale):
    """One pipeline step's two calls: the ControlNet (guidance only if its own guidance_embeds), then the transformer with its samples.
    scale == 0: the plain transformer (the zeros the samples would be add nothing)."""
    if scale == 0:
        return R.transformer_forward(sd, cfg, lat, pe, pool, t, img_ids, txt_ids, guidance)
    bs, ss = _bf16_side(lambda: controlnet_forward_ref(sd_cn, cfg_cn, lat, cond, mode, pe, pool, t, img_ids, txt_ids,
                                                       guidance if cfg_cn.guidance_embeds else None, scale))
    return transformer_forward_ref(sd, cfg, lat, pe, pool, t, img_ids, txt_ids, guidance, bs, ss)


def denoise_ref(sd, cfg, sd_cn, cfg_cn, lat, cond, mode, pe, pool, h2, w2, n, scales, guidance_scale=3.5):
    """FluxControlNetPipeline's loop on packed latents [1, S, 64] with the packed control latents [1, S, 64]; scales: one per step."""
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
        v = controlled_forward_ref(sd, cfg, sd_cn, cfg_cn, x, cond, mode, pe, pool, t / 1000, img_ids, txt_ids, guidance, scales[i])
        x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
    return x


def inputs(cfg, S, T, seed):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(S, LAT, generator=g).bfloat16()
    cond = torch.randn(S, LAT, generator=g).bfloat16()
    cond2 = torch.randn(S, LAT, generator=g).bfloat16()
    pe = torch.randn(T, cfg.joint_attention_dim, generator=g).bfloat16()
    pool = torch.randn(cfg.pooled_projection_dim, generator=g).bfloat16()
    return lat, cond, cond2, pe, pool


# the cases of the GPU tests: (n_d, n_s, num_mode, mode)
CASES = {"1x2": (1, 2, 0, None), "2x0": (2, 0, 0, None), "2x3_union": (2, 3, 2, 1)}
H2, W2, T_TXT, SCALE = 6, 5, 11, 0.7
SEED_MAIN, SEED_CN, SEED_IN = 4, 7, 31


def build_controlnet(cfg_cn, sd_cn, num_mode=0, **caps):
    from thinkdiff.models.flux_controlnet import FluxControlNetConfig, FluxControlNetModel
    caps = {**dict(max_img_tokens=512, max_txt_tokens=128, max_steps=8), **caps}
    m = FluxControlNetModel(FluxControlNetConfig(
        in_channels=cfg_cn.in_channels, num_layers=cfg_cn.num_layers, num_single_layers=cfg_cn.num_single_layers,
        num_attention_heads=cfg_cn.num_attention_heads, joint_attention_dim=cfg_cn.joint_attention_dim,
        pooled_projection_dim=cfg_cn.pooled_projection_dim, guidance_embeds=cfg_cn.guidance_embeds, num_mode=num_mode or None), **caps)
    m.load_state_dict(sd_cn)
    return m
