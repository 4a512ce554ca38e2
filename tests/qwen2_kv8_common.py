"""CPU restatement of the e4m3 KV-cache format of the Qwen2-VL decode engine (include/thinkdiff_hip.h, "e4m3 KV cache"), shared by
tests/test_qwen2_kv8_cpu.py and tests/test_qwen2_kv8_gpu.py.

Format: the weight format of tests/qwen2_w8_common.py applied to every 128-wide head vector x of a cache row (the rotated k | v row of 2 Hkv vectors):
  amax = max |x_d|;  e = the smallest integer with amax 2^-e <= 448, clamped to [-40, 40], 0 for an all-zero vector;
  q_d = e4m3_rne(x_d 2^-e);  x^_d = q_d 2^e.
`qwen2_w8_common.quantize_rows` on the [rows x heads, 128] view IS that restatement; this module adds the row layout (bytes plane, scale plane), the
corner-case vectors, and a restatement of the oracle's decoder loop that rounds every new rotated k, v through a given function before anybody reads it.
"""
import torch
import torch.nn.functional as F

import qwen2_w8_common as W
from oracle import qwen2vl_ref as Q


def quantize_kv_rows(kv, heads):
    """kv [rows, heads * 128] (any float dtype) -> (bytes uint8 [rows, heads * 128], scale fp32 [rows, heads] = 2^e, kv_hat fp32 [rows, heads * 128],
    e int32 [rows, heads])."""
    rows = kv.shape[0]
    assert kv.shape == (rows, heads * 128)
    q, scale, hat, e = W.quantize_rows(kv.reshape(rows * heads, 128))
    return q.reshape(rows, heads * 128), scale.reshape(rows, heads), hat.reshape(rows, heads * 128), e.reshape(rows, heads)


def dequantize_kv_rows(q_u8, scale):
    rows, heads = scale.shape
    return W.dequantize(q_u8.reshape(rows * heads, 128), scale.reshape(rows * heads)).reshape(rows, heads * 128)


def kv_round(x):
    """x [..., 128] -> x^ in x's dtype: every 128-wide vector of the last axis through the format (x^ is exact in bf16, so in any wider dtype too)."""
    hat = W.quantize_rows(x.reshape(-1, 128))[2]
    return hat.reshape(x.shape).to(x.dtype)


def identity(x):
    return x


def edge_kv_rows(rows, heads, seed=0):
    """bf16 [rows, heads * 128]: qwen2_w8_common.edge_rows on the head vectors -- magnitudes 2^-12 .. 2^12 from vector to vector, vector 0 all zero, vector 1
    a single non-zero, vector 2 with a maximum of exactly 448 x 2^3, vector 3 just above it."""
    return W.edge_rows(rows * heads, 128, seed=seed).reshape(rows, heads * 128)


def decoder_layer(sd, cfg, i, h, cos, sin, past_k, past_v, kv_round):
    """oracle.qwen2vl_ref.decoder_layer with the NEW rotated k and v passed through kv_round before the attention and before they are returned."""
    p = f"model.layers.{i}."
    n = h.shape[0]
    Hq, Hkv, hd = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim
    x = Q.rms_norm(h, sd[p + "input_layernorm.weight"], cfg.rms_eps)
    q = F.linear(x, sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.q_proj.bias"]).view(n, Hq, hd).transpose(0, 1)
    k = F.linear(x, sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.k_proj.bias"]).view(n, Hkv, hd).transpose(0, 1)
    v = F.linear(x, sd[p + "self_attn.v_proj.weight"], sd[p + "self_attn.v_proj.bias"]).view(n, Hkv, hd).transpose(0, 1)
    q = q * cos[None] + Q.rotate_half(q) * sin[None]
    k = k * cos[None] + Q.rotate_half(k) * sin[None]
    k, v = kv_round(k), kv_round(v)
    if past_k is not None:
        k, v = torch.cat([past_k, k], dim=1), torch.cat([past_v, v], dim=1)
    kk = k.repeat_interleave(Hq // Hkv, dim=0)
    vv = v.repeat_interleave(Hq // Hkv, dim=0)
    s = torch.matmul(q, kk.transpose(1, 2)) * (hd ** -0.5)
    nt = k.shape[1]
    mask = torch.arange(nt)[None, :] > (torch.arange(n)[:, None] + (nt - n))
    s = s.masked_fill(mask[None], torch.finfo(s.dtype).min)
    a = torch.softmax(s, dim=-1, dtype=torch.float32).to(q.dtype)
    o = torch.matmul(a, vv).transpose(0, 1).reshape(n, Hq * hd)
    h = h + F.linear(o, sd[p + "self_attn.o_proj.weight"])
    x = Q.rms_norm(h, sd[p + "post_attention_layernorm.weight"], cfg.rms_eps)
    m = F.linear(F.silu(F.linear(x, sd[p + "mlp.gate_proj.weight"])) * F.linear(x, sd[p + "mlp.up_proj.weight"]), sd[p + "mlp.down_proj.weight"])
    return h + m, k, v


def text_model_hidden(sd, cfg, position_ids, token_ids=None, inputs_embeds=None, past=None, kv_round=identity):
    """oracle.qwen2vl_ref.text_model_hidden over decoder_layer above: (model.norm(h) [n, D], [(k, v) per layer]) with every cached k, v rounded."""
    h = F.embedding(token_ids, sd["model.embed_tokens.weight"]) if inputs_embeds is None else inputs_embeds
    cos, sin = Q.mrope_cos_sin(position_ids, cfg, h.dtype)
    kv = []
    for i in range(cfg.num_layers):
        pk, pv = past[i] if past is not None else (None, None)
        h, k, v = decoder_layer(sd, cfg, i, h, cos, sin, pk, pv, kv_round)
        kv.append((k, v))
    return Q.rms_norm(h, sd["model.norm.weight"], cfg.rms_eps), kv


# ---- the decode attention's test problem ------------------------------------------------------------------------------------------------------
MUTANTS = ("k_scale_from_v", "scale_of_next_row", "scale_of_other_head", "no_scale")


def attention_case(Hq, Hkv, Skv, B, dom, vmode, seed, lens=None):
    """One decode-attention problem over an e4m3 cache.  Head-vector magnitudes span 2^-6 .. 2^6 from row to row and head to head (k and v
    independently); q is N(0, 1) / 16 so that the scores stay spread (their deviation is |k|'s scale / 16 .. 4).  vmode 'big': v x 2^8; 'offset': v + 500.
    dom: None or the key index made dominant for every q head of its kv head.  Returns a dict with q bf16 [B, Hq*128], the planes as the CPU
    restatement quantises them (bytes [B, Skv, 2 Hkv 128], scale [B, Skv, 2 Hkv]) and lens (int list, every entry Skv unless given)."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Hq * 128, generator=g) / 16).bfloat16()
    expo = torch.randint(-6, 7, (B, Skv, 2 * Hkv), generator=g)
    expo.view(-1)[0], expo.view(-1)[-1] = -6, 6
    x = torch.randn(B, Skv, 2 * Hkv, 128, generator=g) * torch.exp2(expo.float())[..., None]
    if vmode == "big":
        x[:, :, Hkv:] *= 256.0
    elif vmode == "offset":
        x[:, :, Hkv:] += 500.0
    if dom is not None:
        qg = q.float().reshape(B, Hkv, Hq // Hkv, 128).sum(dim=2)      # [B, Hkv, 128]
        x[:, dom, :Hkv] = 768.0 * qg
    x = x.bfloat16().reshape(B * Skv, 2 * Hkv * 128)
    qb, sc, hat, _ = quantize_kv_rows(x, 2 * Hkv)
    return {"q": q, "bytes": qb.reshape(B, Skv, 2 * Hkv * 128), "scale": sc.reshape(B, Skv, 2 * Hkv), "lens": list(lens) if lens is not None else [Skv] * B,
            "Hq": Hq, "Hkv": Hkv, "Skv": Skv, "B": B}


def mutant_scales(scale, Hkv, which):
    """The scale plane [B, Skv, 2 Hkv] a wrong kernel would apply; None where the mutant cannot differ structurally (one row, one head)."""
    B, Skv, _ = scale.shape
    if which is None:
        return scale
    if which == "k_scale_from_v":
        return torch.cat([scale[:, :, Hkv:], scale[:, :, Hkv:]], dim=2)
    if which == "scale_of_next_row":
        return None if Skv == 1 else torch.roll(scale, -1, dims=1)
    if which == "scale_of_other_head":
        return None if Hkv == 1 else scale[:, :, torch.arange(2 * Hkv) ^ 1]
    if which == "no_scale":
        return torch.ones_like(scale)
    raise ValueError(which)


def attention_ref64(case, scale_plane=None):
    """float64 decode attention over the dequantised cache (bytes x scale_plane, default the case's own): [B, Hq*128]; and max |v^| per (B, Hq*128)
    column's kv head over the visible keys."""
    Hq, Hkv, Skv, B = case["Hq"], case["Hkv"], case["Skv"], case["B"]
    sc = case["scale"] if scale_plane is None else scale_plane
    vals = case["bytes"].reshape(B, Skv, 2 * Hkv, 128).view(torch.float8_e4m3fn).double() * sc.double()[..., None]
    k = vals[:, :, :Hkv].permute(0, 2, 1, 3).repeat_interleave(Hq // Hkv, dim=1)      # [B, Hq, Skv, 128]
    v = vals[:, :, Hkv:].permute(0, 2, 1, 3).repeat_interleave(Hq // Hkv, dim=1)
    qh = case["q"].double().reshape(B, Hq, 1, 128)
    s = (qh @ k.transpose(-1, -2)) / (128 ** 0.5)                                     # [B, Hq, 1, Skv]
    lens = torch.tensor(case["lens"])
    hidden = torch.arange(Skv)[None, :] >= lens[:, None]                              # [B, Skv]
    s = s.masked_fill(hidden[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).reshape(B, Hq * 128)
    vmax = v.abs().masked_fill(hidden[:, None, :, None], 0.0).amax(dim=(2, 3))        # [B, Hq]
    return o, vmax.repeat_interleave(128, dim=1)


def attention_tol(ref, vmax):
    """The bound tests/test_attention_gpu.py::test_decode_against_cache derives for the bf16 decode kernel: one bf16 ulp of the reference + 2^-12 max |v^|
    of the kv head (exact operands, fp32 softmax and sums, one rounding: the same arithmetic class)."""
    a = ref.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7) + 2.0 ** -12 * vmax


def mutant_margins(case, ref, tol):
    """{mutant: max |ref_mutant - ref| / tol, or None where the mutant cannot differ}: how far the fp64 reference moves when the scales are misapplied."""
    out = {}
    for m in MUTANTS:
        sp = mutant_scales(case["scale"], case["Hkv"], m)
        out[m] = None if sp is None else float(((attention_ref64(case, sp)[0] - ref).abs() / tol).max())
    return out


# (Hq, Hkv, Skv, batch, dominant key, v mode, mutants the case CANNOT tell from the true scales).  A case covers a mutant when the fp64 reference moves by at
# least 10 x the tolerance under it.  What is not covered, and why: one cached key has no next row and its softmax weight is 1 whatever k is; one kv head
# has no other head; under 'offset' every v vector is 500 + noise and so carries the scale 2^1, and a dominant key (768 x the q heads' sum: a score in the
# hundreds) stays dominant under any of the k scales in play -- then neither the v column's scale for k nor the other head's scale changes anything.
DECODE8_CASES = [
    (12, 2, 1, 70, None, "randn", ("k_scale_from_v", "scale_of_next_row")),
    (28, 4, 2, 3, "last_key", "big", ()),
    (4, 4, 15, 3, "first", "offset", ("k_scale_from_v", "scale_of_other_head")),
    (7, 1, 16, 70, "last_slot", "randn", ("scale_of_other_head",)),
    (12, 2, 17, 3, "last_key", "big", ()),
    (28, 4, 63, 1, "first", "randn", ()),
    (7, 1, 64, 3, "last_slot", "offset", ("k_scale_from_v", "scale_of_other_head")),
    (4, 4, 65, 70, "last_key", "randn", ()),
    (12, 2, 300, 70, None, "big", ()),
    (28, 4, 1025, 3, "last_key", "offset", ()),
    (7, 1, 8192, 1, "first", "big", ("scale_of_other_head",)),
]


def decode8_problem(Hq, Hkv, Skv, B, dom, vmode, lens=None):
    pos = {None: None, "first": 0, "last_slot": min(15, Skv - 1), "last_key": Skv - 1}[dom]
    return attention_case(Hq, Hkv, Skv, B, pos, vmode, seed=Skv * 131 + B * 7 + Hq, lens=lens)


def check_mutant_margins(case, ref, tol, uncovered, what):
    """The condition on the inputs: every mutant the case is listed to cover moves the fp64 reference by >= 10 x the tolerance.  Prints the margins."""
    margins = mutant_margins(case, ref, tol)
    print(f"{what}: mutant margins (x tolerance) " + ", ".join(f"{m} {'n/a' if v is None else format(v, '.3g')}" for m, v in margins.items())
          + (f"; not covered: {', '.join(uncovered)}" if uncovered else ""))
    for m, v in margins.items():
        if m not in uncovered:
            assert v is not None and v >= 10.0, f"{what}: the inputs cannot tell mutant {m} from the true scales (margin {v})"
    return margins
