"""Test-local CPU restatement of several FLUX ControlNets on one transformer, on top of tests/controlnet_common.py; shared by
test_multi_controlnet_cpu.py and test_flux_multi_controlnet_gpu.py.

**Parity unpinned**: restated from the published diffusers sources (`controlnet_flux.py` FluxMultiControlNetModel.forward,
`pipeline_flux_controlnet.py` __call__ with a FluxMultiControlNetModel, `transformer_flux.py`); the spec is the docstring of
thinkdiff/models/flux_controlnet.py.  For the nets k = 0 .. K-1 in list order, at one step with conditioning scale c_k:

    s_k[i] = sample_k[i] * c_k                     (a tensor times a Python float: in bf16 the product of the fp32 values rounds once)
    acc[i] = s_0[i];  acc[i] = acc[i] + s_k[i]     for k = 1 .. K-1: a left fold, every add a tensor op of the dtype (bf16: one rounding each)
    hidden = hidden + acc[idx]                     image rows only, behind double block i / single block i

Two deliberate deviations from diffusers, both the engine's: every net takes ITS OWN index `idx_k = i // ceil(n_blocks / n_samples_k)`
(diffusers zips the nets' sample lists and truncates when the counts differ; with equal counts the two agree) and a net without
single-block samples takes no part in the single-block sums; a net whose scale at the step is 0 is left out (not run, not folded).
Every statement runs on tensors of the dtype it is given (bf16 as the pipeline does, fp32 for the error yardstick)."""
import torch
import torch.nn.functional as F

import controlnet_common as C
from oracle import flux_ref as R


def net(sd, cfg, cond, mode, scale):
    """One entry of the list: the ControlNet's weights and config, ITS control latents [B, S_img, 64], mode and scale at the step."""
    return dict(sd=sd, cfg=cfg, cond=cond, mode=mode, scale=scale)


def fold(samples):
    """Left fold in list order, one tensor add (one rounding in bf16) per step; None for an empty list."""
    acc = None
    for s in samples:
        acc = s if acc is None else acc + s
    return acc


def transformer_forward_multi_ref(sd, cfg, hidden, enc, pooled, timestep, img_ids, txt_ids, guidance, block_lists, single_lists):
    """FluxTransformer2DModel.forward with the scaled samples of several nets: block_lists[k] / single_lists[k] are net k's lists (a net
    without single samples gives an empty one); behind each block the fold of the nets' indexed samples is added once."""
    dt = hidden.dtype
    hidden = R._lin(sd, "x_embedder", hidden)
    timestep = timestep.to(dt) * 1000
    guidance = guidance.to(dt) * 1000 if guidance is not None else None
    temb = R.time_text_embed(sd, cfg, timestep, guidance, pooled)
    enc = R._lin(sd, "context_embedder", enc)
    cos, sin = R.rope_tables(torch.cat([txt_ids, img_ids], dim=0), cfg.axes_dims_rope)
    for i in range(cfg.num_layers):
        enc, hidden = R.double_block(sd, cfg, i, hidden, enc, temb, cos, sin)
        acc = fold([bs[C.sample_index(i, cfg.num_layers, len(bs))] for bs in block_lists if bs])
        if acc is not None:
            hidden = hidden + acc
    T = enc.shape[1]
    hidden = torch.cat([enc, hidden], dim=1)
    for i in range(cfg.num_single_layers):
        hidden = R.single_block(sd, cfg, i, hidden, temb, cos, sin)
        acc = fold([ss[C.sample_index(i, cfg.num_single_layers, len(ss))] for ss in single_lists if ss])
        if acc is not None:
            hidden = torch.cat([hidden[:, :T], hidden[:, T:] + acc], dim=1)
    hidden = hidden[:, T:]
    scale, shift = R._lin(sd, "norm_out.linear", F.silu(temb).to(dt)).chunk(2, dim=1)
    hidden = R._ln(hidden) * (1 + scale)[:, None, :] + shift[:, None, :]
    return R._lin(sd, "proj_out", hidden)


def multi_controlled_forward_ref(sd, cfg, nets, lat, pe, pool, t, img_ids, txt_ids, guidance):
    """One pipeline step: every net whose scale is not 0, in list order (guidance only if its own guidance_embeds), then the transformer
    with the fold of their scaled samples.  No active net: the plain transformer."""
    active = [n for n in nets if n["scale"] != 0]
    if not active:
        return R.transformer_forward(sd, cfg, lat, pe, pool, t, img_ids, txt_ids, guidance)
    bl, sl = [], []
    for n in active:
        bs, ss = C._bf16_side(lambda n=n: C.controlnet_forward_ref(n["sd"], n["cfg"], lat, n["cond"], n["mode"], pe, pool, t, img_ids, txt_ids,
                                                                  guidance if n["cfg"].guidance_embeds else None, n["scale"]))
        bl.append(bs)
        sl.append(ss)
    return transformer_forward_multi_ref(sd, cfg, lat, pe, pool, t, img_ids, txt_ids, guidance, bl, sl)


def multi_denoise_ref(sd, cfg, nets, lat, pe, pool, h2, w2, n, tables, guidance_scale=3.5):
    """The pipeline's loop on packed latents [1, S, 64]; tables[k][i]: net k's scale at step i (the `scale` of each entry of `nets` is ignored)."""
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
        step_nets = [{**nk, "scale": tables[k][i]} for k, nk in enumerate(nets)]
        v = multi_controlled_forward_ref(sd, cfg, step_nets, x, pe, pool, t / 1000, img_ids, txt_ids, guidance)
        x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
    return x


def _per_net(v, K):
    return list(v) if isinstance(v, (list, tuple)) else [v] * K


def keep_tables(n, K, start=0.0, end=1.0):
    """[ext] pipeline_flux_controlnet.py with K nets: controlnet_keep[i][k] = 1.0 - float(i / n < start_k or (i + 1) / n > end_k), here per
    net (keep_tables(..)[k][i]); start / end one number for all nets or a list of K."""
    st, en = _per_net(start, K), _per_net(end, K)
    return [C.keep_schedule(n, st[k], en[k]) for k in range(K)]


def scale_tables(n, K, scale=1.0, start=0.0, end=1.0):
    """Net k's per-step table: scale_k * keep_k[i]."""
    sc = _per_net(scale, K)
    return [[float(sc[k]) * kp for kp in row] for k, row in enumerate(keep_tables(n, K, start, end))]


# the two nets of the GPU tests: case "1x2" on `cond` at 0.7 and case "2x3_union" (mode 1) on `cond2` at 0.45 -- sample counts (1, 2) against
# (2, 3), so the per-net index rule is exercised behind both kinds of block
NETS = (("1x2", "cond", 0.7), ("2x3_union", "cond2", 0.45))
SEED_CN2 = C.SEED_CN + 4      # the second net's weights are its own
