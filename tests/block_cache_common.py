"""Test-local CPU restatement of the first-block cache, shared by test_block_cache_cpu.py and test_block_cache_gpu.py.

**Parity unpinned**: restated from the published diffusers >= 0.33 source (`hooks/first_block_cache.py`) on top of oracle/flux_ref.py; the spec is
the comment above `td_flux_set_block_cache` in include/thinkdiff_hip.h.  Per forward of a context with the cache on:

    h0 = x_embedder(cat([latents, ref]));  h1 = double block 0 of it         (the image rows: latents, then reference tokens)
    r = dt(h1 - h0);  metric = sum |r - r_prev| / sum |r_prev|               sums and ratio in fp64 (diffusers: bf16 means and a bf16 ratio)
    computed (no r_prev | the rule says so):  r_prev <- r, the remaining blocks run, tail = dt(h_final - h1) on the latent rows
    skipped:                                  h = dt(h1 + tail) on the latent rows
    then the final AdaLayerNorm and proj_out on the latent rows.

Runs in any dtype: bf16 is the pipeline's arithmetic, float64 the exact version of the same graph (no rounding where `dt(...)` stands)."""
import math

import torch
import torch.nn.functional as F

from oracle import flux_ref as R


def _up(t):
    return t if t.dtype == torch.float64 else t.float()


class CacheState:
    """What one context carries from forward to forward, and its log."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.r_prev = None
        self.tail = None
        self.count = 0
        self.metrics, self.computed = [], []


def forward(sd, cfg, st, lat, pe, pool, t, img_ids, txt_ids, guidance, threshold=None, schedule=None, ref=None, ref_ids=None, tail_use=None):
    """One transformer forward under the cache.  lat [1, S, 64]; t [1] in [0, 1] (the pipeline's t / 1000); exactly one of threshold / schedule.
    tail_use (discriminators only): "drop" = a skipped forward adds nothing; a tensor = it adds that tail instead of the state's."""
    dt = lat.dtype
    S = lat.shape[1]
    x, ids = lat, img_ids
    if ref is not None and ref.shape[1] > 0:
        x = torch.cat([lat, ref.to(dt)], dim=1)
        ids = torch.cat([img_ids, ref_ids.to(img_ids.dtype)], dim=0)
    hidden = R._lin(sd, "x_embedder", x)
    timestep = t.to(dt) * 1000
    g = guidance.to(dt) * 1000 if guidance is not None else None
    temb = R.time_text_embed(sd, cfg, timestep, g, pool)
    enc = R._lin(sd, "context_embedder", pe)
    cos, sin = R.rope_tables(torch.cat([txt_ids, ids], dim=0), cfg.axes_dims_rope)
    h0 = hidden
    enc, hidden = R.double_block(sd, cfg, 0, hidden, enc, temb, cos, sin)
    h1 = hidden
    r = (_up(h1) - _up(h0)).to(dt)
    if st.r_prev is None:
        metric = math.inf
    else:
        den = float(st.r_prev.double().abs().sum())
        metric = float((_up(r) - _up(st.r_prev)).double().abs().sum()) / den if den > 0 else math.inf
    if st.r_prev is None or math.isinf(metric):
        compute = True
    elif schedule is not None:
        compute = st.count >= len(schedule) or bool(schedule[st.count])
    else:
        compute = metric > threshold
    st.count += 1
    st.metrics.append(metric)
    st.computed.append(compute)
    if compute:
        st.r_prev = r
        for i in range(1, cfg.num_layers):
            enc, hidden = R.double_block(sd, cfg, i, hidden, enc, temb, cos, sin)
        T = enc.shape[1]
        hidden = torch.cat([enc, hidden], dim=1)
        for i in range(cfg.num_single_layers):
            hidden = R.single_block(sd, cfg, i, hidden, temb, cos, sin)
        hidden = hidden[:, T:T + S]
        st.tail = (_up(hidden) - _up(h1[:, :S])).to(dt)
    else:
        tail = st.tail if tail_use is None else tail_use
        hidden = h1[:, :S] if isinstance(tail, str) else (_up(h1[:, :S]) + _up(tail)).to(dt)
    scale, shift = R._lin(sd, "norm_out.linear", F.silu(temb).to(dt)).chunk(2, dim=1)
    hidden = R._ln(hidden) * (1 + scale)[:, None, :] + shift[:, None, :]
    return R._lin(sd, "proj_out", hidden)


def scalars(dt, t_bf16_exact: float, guidance_scale: float = 3.5):
    """(t, guidance) tensors for `forward` in dtype dt that make every dtype see the scalars the bf16 pipeline sees."""
    t = torch.tensor([t_bf16_exact]).bfloat16()
    if dt == torch.bfloat16:
        return t, torch.tensor([guidance_scale])
    return t.to(dt), torch.tensor([float((torch.tensor([guidance_scale]).bfloat16() * 1000).float()) / 1000], dtype=dt)


def denoise(sd, cfg, lat, pe, pool, h2, w2, n, threshold=None, schedule=None, guidance_scale=3.5, state=None):
    """oracle.flux_ref.denoise with `forward` in place of the transformer; returns (final latents, state).  In bf16 every statement is
    R.denoise's; in a wider dtype the timesteps are the scalars the bf16 pipeline's sinusoids see and the Euler step is exact."""
    dt = lat.dtype
    st = state or CacheState()
    st.reset()      # (diffusers resets its cache state per pipeline call)
    S = lat.shape[1]
    sig = R.make_sigmas(n, S)
    sig_t = torch.from_numpy(sig)
    img_ids = R.latent_image_ids(h2, w2).to(dt)
    txt_ids = torch.zeros(pe.shape[1], 3).to(dt)
    x = lat
    for i in range(n):
        if dt == torch.bfloat16:
            t = ((torch.from_numpy(sig[:-1]) * 1000.0)[i].expand(1).to(dt)) / 1000
            g = torch.full([1], guidance_scale, dtype=torch.float32) if cfg.guidance_embeds else None
        else:
            t = torch.tensor([R.effective_timestep(float(sig[i]) * 1000.0, torch.bfloat16) / 1000], dtype=dt)
            g = scalars(dt, 0.5, guidance_scale)[1] if cfg.guidance_embeds else None
        v = forward(sd, cfg, st, x, pe, pool, t, img_ids, txt_ids, g, threshold=threshold, schedule=schedule)
        if dt == torch.bfloat16:
            x = (x.to(torch.float32) + (sig_t[i + 1] - sig_t[i]) * v).to(v.dtype)
        else:
            x = x + (sig_t[i + 1] - sig_t[i]).to(dt) * v
    return x, st


def rel_rmse(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def parse_schedule(s: str):
    """'CsC' -> [1, 0, 1]"""
    return [1 if c == "C" else 0 for c in s]


# ---- the GPU tests' fixture (the issue's: 3 + 3 layers, 16 x 16 latent tokens, 40 text tokens, weights seed 7, inputs seed 3) -------------------------
H2 = W2 = 16
T_TXT = 40
N_STEPS = 8


def fixture():
    cfg = R.tiny_config(num_layers=3, num_single_layers=3)
    sd = R.init_weights(cfg, seed=7)
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(1, H2 * W2, 64, generator=g).bfloat16()
    pe = torch.randn(1, T_TXT, cfg.joint_attention_dim, generator=g).bfloat16()
    pool = torch.randn(1, cfg.pooled_projection_dim, generator=g).bfloat16()
    return cfg, sd, lat, pe, pool


def widen(sd, *tensors, dt=torch.float64):
    return {k: v.to(dt) for k, v in sd.items()}, [t.to(dt) for t in tensors]


def build_engine(cfg, sd, **caps):
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig
    caps = {**dict(max_img_tokens=512, max_txt_tokens=64, max_steps=8), **caps}
    m = FluxTransformer2DModel(FluxTransformerConfig(
        in_channels=cfg.in_channels, num_layers=cfg.num_layers, num_single_layers=cfg.num_single_layers,
        num_attention_heads=cfg.num_attention_heads, joint_attention_dim=cfg.joint_attention_dim,
        pooled_projection_dim=cfg.pooled_projection_dim, guidance_embeds=cfg.guidance_embeds), **caps)
    m.load_state_dict(sd)
    return m


def prepare(m, pe, pool, n, h2=H2, w2=W2):
    """set_condition + the n-step schedule of `denoise`; returns the sigmas."""
    from thinkdiff.models.flux_transformer import effective_scalar
    sig = R.make_sigmas(n, h2 * w2)
    m.set_condition(pe[0].cuda(), pool[0].cuda(), R.latent_image_ids(h2, w2))
    m.set_timesteps([effective_scalar(float(s) * 1000.0, torch.bfloat16) for s in sig[:-1]], float((torch.tensor([3.5]).bfloat16() * 1000).float()))
    return sig
