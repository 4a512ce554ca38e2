"""Test-local CPU restatement of the FLUX IP-Adapter, shared by test_ip_adapter_cpu.py and test_flux_ip_adapter_gpu.py.

**Parity unpinned**: restated from the published diffusers sources (`attention_processor.FluxIPAdapterJointAttnProcessor2_0`,
`transformer_flux.FluxTransformerBlock.forward`, `embeddings.ImageProjection`, `loaders/transformer_flux.py`), composed from oracle/flux_ref.py;
the spec is the docstring of thinkdiff/models/flux_ip_adapter.py.  Every statement runs on tensors of the dtype it is given (bf16 as the
pipeline does, fp32 for the error yardstick).

The double block with IP is `R.double_block(...)` followed by recomputing `ip_query` from the block's INPUTS and adding `ip`: bit-equal to doing it
inside (`R._lin` is deterministic), and with no adapter it IS the oracle's block.

Main model: the ControlNet tests' (`R.tiny_config(num_layers=2, num_single_layers=3)`, D = 512, 4 heads, 6 x 5 latent tokens, T = 11, seed 4).
Adapter fixture: E = 32; proj.weight std 0.05, proj.bias 0.02, norm.weight 1 + 0.1 randn, norm.bias 0.05, to_k_ip 0.02 (weight and bias),
to_v_ip **0.004**, scale 0.7.  At these stds IP moves the output by 0.17 - 0.27 rel-RMSE, another image prompt by 0.25 - 0.37, while the
reference's own bf16-vs-fp32 distance stays the plain model's (0.027 - 0.028 vs 0.0285); at to_v_ip std 0.02 the IP term swamps the output
(0.7 - 0.9), which would hide errors of the main path."""
import torch
import torch.nn.functional as F

from oracle import flux_ref as R

LAT = 64
BF = torch.bfloat16
E_DIM = 32
H2, W2, T_TXT, SCALE = 6, 5, 11, 0.7
SEED_MAIN, SEED_IP, SEED_IN = 4, 11, 31


def rel_rmse(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def main_config():
    return R.tiny_config(num_layers=2, num_single_layers=3)


def ip_init_weights(cfg, num_tokens, seed=SEED_IP, v_std=0.004, E=E_DIM, dtype=BF):
    """Seeded synthetic adapter in the diffusers form {"image_proj": {...}, "ip_adapter": {"{i}.to_k_ip.weight": ...}}."""
    g = torch.Generator().manual_seed(seed)
    J, D = cfg.joint_attention_dim, cfg.inner_dim
    rn = lambda *shape: torch.randn(*shape, generator=g)
    proj = {"proj.weight": 0.05 * rn(num_tokens * J, E), "proj.bias": 0.02 * rn(num_tokens * J),
            "norm.weight": 1.0 + 0.1 * rn(J), "norm.bias": 0.05 * rn(J)}
    blocks = {}
    for i in range(cfg.num_layers):
        blocks[f"{i}.to_k_ip.weight"] = 0.02 * rn(D, J)
        blocks[f"{i}.to_k_ip.bias"] = 0.02 * rn(D)
        blocks[f"{i}.to_v_ip.weight"] = v_std * rn(D, J)
        blocks[f"{i}.to_v_ip.bias"] = v_std * rn(D)
    return {"image_proj": {k: v.to(dtype) for k, v in proj.items()}, "ip_adapter": {k: v.to(dtype) for k, v in blocks.items()}}


def cast(ip_sd, dtype):
    return {part: {k: v.to(dtype) for k, v in d.items()} for part, d in ip_sd.items()}


def image_embeds(n_img, seed, E=E_DIM):
    return torch.randn(n_img, E, generator=torch.Generator().manual_seed(seed)).bfloat16()


def image_tokens(ip_sd, cfg, embeds):
    """[ext] embeddings.ImageProjection.forward: embeds [n_img, E] -> tokens [n_img * num_tokens, J]."""
    p = ip_sd["image_proj"]
    J = cfg.joint_attention_dim
    x = F.linear(embeds.to(p["proj.weight"].dtype), p["proj.weight"], p["proj.bias"]).reshape(-1, J)
    return F.layer_norm(x, (J,), p["norm.weight"], p["norm.bias"], eps=1e-5)


def block_kv(ip_sd, i, tokens):
    """K_i, V_i [n_keys, D] of double block i."""
    b = ip_sd["ip_adapter"]
    return (F.linear(tokens, b[f"{i}.to_k_ip.weight"], b[f"{i}.to_k_ip.bias"]), F.linear(tokens, b[f"{i}.to_v_ip.weight"], b[f"{i}.to_v_ip.bias"]))


def ip_query(sd, cfg, i, hidden, temb):
    """The image stream's norm_q(to_q(norm_hidden)) of double block i, from the block's inputs; [B, H, S, 128], before RoPE."""
    p = f"transformer_blocks.{i}."
    sh_msa, sc_msa = R._lin(sd, p + "norm1.linear", F.silu(temb)).chunk(6, dim=1)[:2]
    n_h = R._ln(hidden) * (1 + sc_msa[:, None]) + sh_msa[:, None]
    return R.rms_norm(R._heads(R._lin(sd, p + "attn.to_q", n_h), cfg.num_attention_heads), sd[p + "attn.norm_q.weight"])


def ip_term(sd, cfg, i, hidden, temb, adapters):
    """[ext] FluxIPAdapterJointAttnProcessor2_0: ip = 0; ip += scale * SDPA(ip_query, K, V) per adapter; None when nothing contributes.
    adapters: (ip_sd, tokens, per-block scales) triples."""
    live = [(a, t, s[i]) for a, t, s in adapters if s[i] != 0]
    if not live:
        return None
    q = ip_query(sd, cfg, i, hidden, temb)
    B, H, S, hd = q.shape
    ip = torch.zeros(B, S, H * hd, dtype=hidden.dtype)
    for ip_sd, tokens, scale in live:
        k, v = block_kv(ip_sd, i, tokens)
        k, v = R._heads(k[None].expand(B, -1, -1), H), R._heads(v[None].expand(B, -1, -1), H)
        o = F.scaled_dot_product_attention(q, k, v, dropout_p=0.0, is_causal=False)
        ip = ip + scale * o.transpose(1, 2).reshape(B, S, H * hd).to(q.dtype)
    return ip


def transformer_forward_ref(sd, cfg, hidden, enc, pooled, timestep, img_ids, txt_ids, guidance, adapters=()):
    """FluxTransformer2DModel.forward with `joint_attention_kwargs={"ip_hidden_states": ...}`; no adapters: R.transformer_forward's statements."""
    dt = hidden.dtype
    hidden = R._lin(sd, "x_embedder", hidden)
    timestep = timestep.to(dt) * 1000
    guidance = guidance.to(dt) * 1000 if guidance is not None else None
    temb = R.time_text_embed(sd, cfg, timestep, guidance, pooled)
    enc = R._lin(sd, "context_embedder", enc)
    cos, sin = R.rope_tables(torch.cat([txt_ids, img_ids], dim=0), cfg.axes_dims_rope)
    for i in range(cfg.num_layers):
        ip = ip_term(sd, cfg, i, hidden, temb, adapters)
        enc, hidden = R.double_block(sd, cfg, i, hidden, enc, temb, cos, sin)
        if ip is not None:
            hidden = hidden + ip
    T = enc.shape[1]
    hidden = torch.cat([enc, hidden], dim=1)
    for i in range(cfg.num_single_layers):
        hidden = R.single_block(sd, cfg, i, hidden, temb, cos, sin)
    hidden = hidden[:, T:]
    scale, shift = R._lin(sd, "norm_out.linear", F.silu(temb).to(dt)).chunk(2, dim=1)
    hidden = R._ln(hidden) * (1 + scale)[:, None, :] + shift[:, None, :]
    return R._lin(sd, "proj_out", hidden)


def make_adapters(cfg, specs, dtype=BF):
    """specs: (ip_sd, embeds [n_img, E], scale: float or per-block list) -> the (ip_sd, tokens, per-block scales) triples in `dtype`."""
    out = []
    for ip_sd, embeds, scale in specs:
        w = cast(ip_sd, dtype)
        s = [float(scale)] * cfg.num_layers if isinstance(scale, (int, float)) else [float(v) for v in scale]
        out.append((w, image_tokens(w, cfg, embeds.to(dtype)), s))
    return out


def denoise_ref(sd, cfg, lat, pe, pool, h2, w2, n, adapters, guidance_scale=3.5):
    """FluxPipeline's loop on packed latents [1, S, 64] with an image prompt (R.denoise's statements around transformer_forward_ref)."""
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
        v = transformer_forward_ref(sd, cfg, x, pe, pool, t / 1000, img_ids, txt_ids, guidance, adapters)
        x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
    return x


def inputs(cfg, S, T, seed=SEED_IN):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(S, LAT, generator=g).bfloat16()
    pe = torch.randn(T, cfg.joint_attention_dim, generator=g).bfloat16()
    pool = torch.randn(cfg.pooled_projection_dim, generator=g).bfloat16()
    return lat, pe, pool


def step_args(lat, pe, pool, dtype, S, T):
    """(lat, pe, pool, t, img_ids, txt_ids, guidance) of a one-step call at the first sigma of a 2-step schedule, bf16 as the pipeline makes them
    or fp32 for the yardstick."""
    t = torch.tensor([float(R.make_sigmas(2, S)[0]) * 1000.0]).bfloat16() / 1000
    ids = R.latent_image_ids(H2, W2)
    if dtype == BF:
        return lat[None], pe[None], pool[None], t, ids.bfloat16(), torch.zeros(T, 3).bfloat16(), torch.tensor([3.5])
    g35 = float((torch.tensor([3.5]).bfloat16() * 1000).float())
    return lat[None].float(), pe[None].float(), pool[None].float(), t.float(), ids, torch.zeros(T, 3), torch.tensor([g35 / 1000])


# ---- the kernel's reference (tests of td_ip_attention_bf16) --------------------------------------------------------------------------------
def kernel_reference(q, k, v, H, norm_w, out_scale):
    """fp64: qn = R.rms_norm(q, w) in bf16 (bit-defined), then softmax and P.V in fp64, times out_scale.  q [rows, H*128], k / v [n, H*128]."""
    rows, n = q.shape[0], k.shape[0]
    qh = q.view(rows, H, 128)
    qn = R.rms_norm(qh, norm_w) if norm_w is not None else qh
    s = torch.einsum("mhd,nhd->hmn", qn.double(), k.view(n, H, 128).double()) * (128 ** -0.5)
    o = torch.einsum("hmn,nhd->mhd", torch.softmax(s, dim=-1), v.view(n, H, 128).double())
    return (o * float(out_scale)).reshape(rows, H * 128)


def kernel_restatement_bf16(q, k, v, H, norm_w, out_scale):
    """The bf16 torch ops of the processor: SDPA on bf16 tensors, then `scale * o`."""
    rows, n = q.shape[0], k.shape[0]
    qh = q.view(rows, H, 128)
    qn = (R.rms_norm(qh, norm_w) if norm_w is not None else qh).transpose(0, 1)[None]
    kh, vh = k.view(n, H, 128).transpose(0, 1)[None], v.view(n, H, 128).transpose(0, 1)[None]
    o = F.scaled_dot_product_attention(qn, kh, vh, dropout_p=0.0, is_causal=False)[0].transpose(0, 1).reshape(rows, H * 128)
    return float(out_scale) * o
