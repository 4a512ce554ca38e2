"""Test-local CPU restatement of FLUX.1 Kontext, shared by test_kontext_cpu.py and test_flux_kontext_gpu.py.

**Parity unpinned**: restated from the published diffusers >= 0.34 source (`pipeline_flux_kontext.py` `prepare_latents` /
`__call__`), on top of oracle/flux_ref.py and vae_encoder_common.py; the spec is the docstring of thinkdiff/models/flux_kontext.py.
Every statement runs on bf16 tensors, as the pipeline does.

The transformer is the plain one (64 / 64): per step it runs on `torch.cat([latents, ref], dim=1)` with
`torch.cat([latent_ids, ref_ids], dim=0)` and the first S rows of its output are the velocity.  The schedule is the latents' own
(`make_sigmas(n, S)`, not S + S_ref).  With a negative branch: `v = v_neg + scale * (v_pos - v_neg)` as three bf16 ops."""
import torch

from oracle import flux_ref as R

LAT = 64


def reference_ids(h2: int, w2: int) -> torch.Tensor:
    """`_prepare_latent_image_ids` with `image_ids[..., 0] = 1`."""
    ids = R.latent_image_ids(h2, w2)
    ids[:, 0] = 1
    return ids


def forward_ref(sd, cfg, lat, ref, pe, pool, t, img_ids, ref_ids, txt_ids, guidance):
    """The oracle on cat([latents, ref]) / cat([img_ids, ref_ids]), first S rows.  ref None: the plain forward."""
    if ref is None or ref.shape[1] == 0:
        return R.transformer_forward(sd, cfg, lat, pe, pool, t, img_ids, txt_ids, guidance)
    x = torch.cat([lat, ref.to(lat.dtype)], dim=1)
    ids = torch.cat([img_ids, ref_ids.to(img_ids.dtype)], dim=0)
    return R.transformer_forward(sd, cfg, x, pe, pool, t, ids, txt_ids, guidance)[:, : lat.shape[1]]


def denoise_ref(sd, cfg, lat, ref, ref_ids, pe, pool, h2, w2, n, guidance_scale=3.5, neg=None, scale=1.0):
    """FluxKontextPipeline's loop on packed latents [1, S, 64] with the reference tokens [1, S_ref, 64] (None: none).
    neg: None, or (negative_prompt_embeds, negative_pooled) -- true CFG with `scale` (a Python float, as in the pipeline)."""
    dt = lat.dtype
    sig = R.make_sigmas(n, lat.shape[1])
    timesteps = torch.from_numpy(sig[:-1]) * 1000.0
    img_ids = R.latent_image_ids(h2, w2).to(dt)
    rid = None if ref is None else ref_ids.to(dt)
    guidance = torch.full([1], guidance_scale, dtype=torch.float32) if cfg.guidance_embeds else None
    sig_t = torch.from_numpy(sig)
    x = lat
    for i in range(n):
        t = timesteps[i].expand(1).to(dt)
        v = forward_ref(sd, cfg, x, ref, pe, pool, t / 1000, img_ids, rid, torch.zeros(pe.shape[1], 3).to(dt), guidance)
        if neg is not None:
            vn = forward_ref(sd, cfg, x, ref, neg[0], neg[1], t / 1000, img_ids, rid, torch.zeros(neg[0].shape[1], 3).to(dt), guidance)
            v = vn + scale * (v - vn)
        x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
    return x


def build_engine(cfg, sd, **caps):
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig
    caps = {**dict(max_img_tokens=512, max_txt_tokens=128, max_steps=8), **caps}
    m = FluxTransformer2DModel(FluxTransformerConfig(
        in_channels=cfg.in_channels, num_layers=cfg.num_layers, num_single_layers=cfg.num_single_layers,
        num_attention_heads=cfg.num_attention_heads, joint_attention_dim=cfg.joint_attention_dim,
        pooled_projection_dim=cfg.pooled_projection_dim, guidance_embeds=cfg.guidance_embeds), **caps)
    m.load_state_dict(sd)
    return m
