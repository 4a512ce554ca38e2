"""Test-local CPU restatement of LoRA on the FLUX transformer, shared by test_lora_cpu.py and test_flux_lora_gpu.py.

**Parity unpinned**: restated from the published peft source (`LoraLayer.forward`: `result + lora_B(lora_A(dropout(x))) * scaling`,
`scaling = lora_alpha / r`; `merge`: `weight + scaling * (lora_B.weight @ lora_A.weight)`) and diffusers' `save_lora_weights` key layout
(`transformer.<module>.lora_A.weight` / `.lora_B.weight`); the spec is the docstring of thinkdiff/models/flux_lora.py.

The model reference is oracle/flux_ref.py, untouched, run on `merged_state_dict`: base weights plus every adapter's update, summed in fp64 and
rounded once."""
import torch

from oracle import flux_ref as R


def block_linears(cfg):
    """The 17 attention / MLP Linears of a 1 + 1 block tiny config (more with more blocks), by module name."""
    mods = []
    for i in range(cfg.num_layers):
        p = f"transformer_blocks.{i}."
        mods += [p + n for n in ("attn.to_q", "attn.to_k", "attn.to_v", "attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj", "attn.to_out.0",
                                 "attn.to_add_out", "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2")]
    for i in range(cfg.num_single_layers):
        p = f"single_transformer_blocks.{i}."
        mods += [p + n for n in ("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp", "proj_out")]
    return mods


def make_lora(cfg, targets, rank, seed, b_std=0.1, prefix="transformer.", alpha=None):
    """A peft-format state dict over the Linears `targets` of a `cfg` transformer: A ~ N(0, 1 / K), B ~ N(0, b_std^2), bf16.
    alpha: None (no alpha keys: scale 1) or a number stored as `<module>.alpha`."""
    g = torch.Generator().manual_seed(seed)
    shapes = R.param_shapes(cfg)
    out = {}
    for mod in targets:
        N, K = shapes[mod + ".weight"]
        out[f"{prefix}{mod}.lora_A.weight"] = (torch.randn(rank, K, generator=g) / K ** 0.5).bfloat16()
        out[f"{prefix}{mod}.lora_B.weight"] = (torch.randn(N, rank, generator=g) * b_std).bfloat16()
        if alpha is not None:
            out[f"{prefix}{mod}.alpha"] = torch.tensor(float(alpha))
    return out


def lora_pairs(lora):
    """{module: (A, B, alpha or None)} of a make_lora dict (either prefix)."""
    out = {}
    for k, v in lora.items():
        k = k[len("transformer."):] if k.startswith("transformer.") else k
        for suf, i in ((".lora_A.weight", 0), (".lora_B.weight", 1), (".alpha", 2)):
            if k.endswith(suf):
                out.setdefault(k[:-len(suf)], [None, None, None])[i] = v
    return {m: tuple(v) for m, v in out.items()}


def merged_state_dict(sd, loras, weights, dtype=torch.bfloat16):
    """W + sum_i w_i (alpha_i / r_i) B_i A_i in fp64, then fp64 -> fp32 (-> bf16 for the bf16 oracle); untouched tensors are cast to `dtype`."""
    acc = {}
    for lora, w in zip(loras, weights):
        for mod, (A, B, alpha) in lora_pairs(lora).items():
            r = A.shape[0]
            s = float(w) * (float(alpha) / r if alpha is not None else 1.0)
            acc[mod] = acc.get(mod, 0) + s * (B.double() @ A.double())
    out = {}
    for k, v in sd.items():
        mod = k[:-len(".weight")] if k.endswith(".weight") else None
        if mod in acc:
            v = (v.double() + acc[mod]).float()
        out[k] = v.to(dtype)
    return out


def rel_rmse(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def forward_ref(sd, cfg, lat, pe, pool, h2, w2, n_steps=2, step=0, dtype=torch.bfloat16, guidance=3.5):
    """The oracle's velocity at schedule step `step` of an n_steps schedule, as the pipeline feeds it (t / 1000 in bf16)."""
    S, T = lat.shape[0], pe.shape[0]
    t = torch.tensor([float(R.make_sigmas(n_steps, S)[step]) * 1000.0]).bfloat16() / 1000
    ids = R.latent_image_ids(h2, w2)
    if dtype == torch.bfloat16:
        return R.transformer_forward(sd, cfg, lat[None], pe[None], pool[None], t.bfloat16(), ids.bfloat16(), torch.zeros(T, 3).bfloat16(),
                                     torch.tensor([guidance]))
    g = torch.tensor([float((torch.tensor([guidance]).bfloat16() * 1000).float()) / 1000])
    return R.transformer_forward(sd, cfg, lat[None].float(), pe[None].float(), pool[None].float(), t.bfloat16().float(), ids, torch.zeros(T, 3), g)
