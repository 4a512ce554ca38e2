"""What the tile attention kernels write, as digests: the record behind a refactor of csrc/attention_bf16.hip / attention_fp8.hip /
attention_common.h (profiles/attention_one_item_body.md).  The GPU tests compare a launch with a reference or with another form of the same
build; this compares two BUILDS: run it from each build's tree.

--out FILE.json   runs a fixed list of launches through thinkdiff._hip (the C ABI of this tree's library; no torch.ops) on seeded inputs and writes one
                  sha256 per launch over its whole output buffer -- three guard rows behind the last row and the pad columns behind the last head
                  included -- plus the int8 plane and the row maxima where the form has them.  Shapes are the smallest at which each path can still go
                  wrong (a ragged last query tile and KV tile, more items than CUs so that items are split over two persistent workgroups, one KV tile
                  per item so that none is); `cus` is read from the device.  Two entries go through an engine because no stand-alone entry reaches
                  their code.  The history references of the e4m3 kernel (ref_in / ref_out): a 3-step denoise of the tiny FLUX model, every step fed
                  the references the step before left; the engine keeps the reference buffers to itself, so the digest is over the final latent,
                  which steps 2 and 3 computed from them.  Per-sequence cache lengths (kv_lens): a batched decode of the tiny Qwen2 model with two
                  lengths -- that launch goes through td_attn_launch to the DECODE kernel (attention_decode.hip); no entry of the library hands
                  kv_lens to the tile kernel, so its kv_lens branch is in no digest.
--compare A B     lists the entries in which two such files differ; exit status 1 if there are any.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "thinkdiff-mlre_amd")):
    sys.path.insert(0, _p)
from thinkdiff import _hip as hip  # noqa: E402

SCALE_LOG2E = (128 ** -0.5) * 1.4426950408889634


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).bfloat16().cuda()


def out2(S, W, pad=8, fill=0.5):
    """[S + 3, W + pad] filled; the launch gets the [S, W] corner.  pad = 4: rows that are no 16-byte multiple (the narrow store)."""
    buf = torch.full((S + 3, W + pad), fill, dtype=torch.bfloat16, device="cuda")
    return buf, buf[:S, :W]


def out3(B, S, W, pad=8, fill=0.5):
    buf = torch.full((B, S + 3, W + pad), fill, dtype=torch.bfloat16, device="cuda")
    return buf, buf[:, :S, :W]


class Variant:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.prev = hip.lib().td_attention_set_variant(self.v)

    def __exit__(self, *a):
        hip.lib().td_attention_set_variant(self.prev)


def current_variant():
    cur = hip.lib().td_attention_set_variant(0)
    hip.lib().td_attention_set_variant(cur)
    return cur


def qkv3(g, B, S, Hq, Hkv):
    d = rand(g, B, S, (Hq + 2 * Hkv) * 128)
    return d[:, :, :Hq * 128], d[:, :, Hq * 128:(Hq + Hkv) * 128], d[:, :, (Hq + Hkv) * 128:]


def joint(seed, B, S, H, pad=8):
    """td_attention_bf16, joint: one [B, S, 3 H 128] projection buffer."""
    q, k, v = qkv3(torch.Generator().manual_seed(seed), B, S, H, H)

    def f():
        buf, o = out3(B, S, H * 128, pad)
        hip.attention(q, k, v, o, H, H)
        return [buf]
    return f


def q8_planes(g, S, W):
    q8 = torch.full((S + 3, W + 16), 77, dtype=torch.int8, device="cuda")
    inv = (torch.rand(S, generator=g) * 60.0 + 20.0).cuda()
    amax = torch.zeros(S + 2, dtype=torch.int32, device="cuda")
    return q8, inv, amax


def joint_forms(seed, S, H):
    """The pre-scaled-q form (variant bit 0x800 of td_attention_bf16), the fixed-reference form (td_attention_joint_prescaled_bf16 with the
    Cauchy-Schwarz bound of the operands) and the int8-output form (td_attention_q8) on one set of operands."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, 3 * H * 128, generator=g)
    x[:, :H * 128] *= SCALE_LOG2E
    x = x.bfloat16()
    W = H * 128
    bound = float(x[:, :W].float().view(S, H, 128).norm(dim=2).amax() * x[:, W:2 * W].float().view(S, H, 128).norm(dim=2).amax())
    d = x.cuda()
    q, k, v = d[:, :W], d[:, W:2 * W], d[:, 2 * W:]
    planes = q8_planes(g, S, W)

    def prescaled():
        buf, o = out3(1, S, W)
        with Variant(current_variant() | 0x800):
            hip.attention(q[None], k[None], v[None], o, H, H)
        return [buf]

    def fixed():
        buf, o = out2(S, W)
        hip.attention_joint_prescaled(q, k, v, o, H, min(bound, 48.0))
        return [buf]

    def int8_out():
        q8, inv, amax = (t.clone() for t in planes)
        hip.attention_q8(q, k, v, q8[:S, :W], inv, amax[:S], H, q_prescaled=True)
        return [q8, amax]
    return prescaled, fixed, int8_out


def plain_grid_cases(cus):
    cases = [("joint_S64_H1", joint(1, 1, 64, 1)), ("joint_S300_H2", joint(2, 1, 300, 2)), ("joint_S300_H2_rows_not_16B", joint(3, 1, 300, 2, pad=4))]
    g = torch.Generator().manual_seed(4)
    q, k, v = qkv3(g, 2, 300, 4, 2)

    def causal_gqa():
        buf, o = out3(2, 300, 4 * 128)
        hip.attention(q, k, v, o, 4, 2, causal=True)
        return [buf]
    cases.append(("causal_gqa_S300_4q2kv_B2", causal_gqa))
    qc, cache = rand(g, 2, 70, 4 * 128), rand(g, 2, 307, 2 * 2 * 128 + 64)

    def cached_prefill():
        buf, o = out3(2, 70, 4 * 128)
        hip.attention(qc, cache[:, :300, :256], cache[:, :300, 256:512], o, 4, 2, causal=True)
        return [buf]
    cases.append(("causal_cached_prefill_Sq70_Skv300", cached_prefill))
    for causal in (False, True):
        qb, kb, vb = rand(g, 70, 4 * 128), rand(g, 132, 2 * 128), rand(g, 132, 2 * 128)
        bias = (torch.randn(4, 70, 132, generator=g) * 2.0).cuda()

        def biased(qb=qb, kb=kb, vb=vb, bias=bias, causal=causal):
            buf, o = out2(70, 4 * 128)
            hip.attention_bias(qb, kb, vb, o, 4, 2, 128 ** -0.5, causal, bias)
            return [buf]
        cases.append((f"bias_dense_Sq70_Skv132_causal{int(causal)}", biased))
    lens = [1, 64, 300, 65]
    S = sum(lens)
    starts = torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32).cuda()
    ps = rand(g, S, (4 + 2 * 2) * 128)
    for causal in (False, True):
        def packed(causal=causal):
            buf, o = out2(S, 4 * 128)
            hip.attention_segments(ps[:, :512], ps[:, 512:768], ps[:, 768:], o, 4, 2, starts, max(lens), causal=causal)
            return [buf]
        cases.append((f"packed_segments_1_64_300_65_causal{int(causal)}", packed))
    pre, fixed, int8_out = joint_forms(5, 300, 2)
    cases += [("prescaled_q_S300_H2", pre), ("fixed_reference_S300_H2", fixed), ("int8_out_S300_H2", int8_out)]
    return [("plain/" + n, f) for n, f in cases]


def streamk_shapes(cus):
    """(name, B, S, H): nearly every item split over two workgroups; one KV tile per item (nothing to split, some workgroups run two items); batched."""
    return [(f"S300_H{cus // 2 + 2}", 1, 300, cus // 2 + 2), (f"S64_H{cus + 4}", 1, 64, cus + 4), (f"B2_S300_H{cus // 4 + 2}", 2, 300, cus // 4 + 2)]


def streamk_cases(cus):
    """Every shape under variant 0 (stream-K), 2 (no XCD remap) and 1 (the plain grid at the same shape)."""
    cases = []
    shapes = streamk_shapes(cus)
    launches = [(name, joint(10 + i, B, S, H)) for i, (name, B, S, H) in enumerate(shapes)]
    forms = joint_forms(20, 300, cus // 2 + 2)
    launches += [(f"{what}_{shapes[0][0]}", f) for what, f in zip(("prescaled_q", "fixed_reference", "int8_out"), forms)]
    for variant in (0, 2, 1):
        for name, f in launches:
            if variant == 1 and not name.startswith(("S", "B")):
                continue      # (the plain-grid forms are covered at S = 300, H = 2)

            def run(f=f, variant=variant):
                with Variant(variant):
                    return f()
            cases.append((f"streamk_shapes/variant{variant}/{name}", run))
    return cases


def fp8_cases(cus):
    cases = []
    g = torch.Generator().manual_seed(30)
    shapes = [(64, 64, 1), (300, 300, 2), (257, 65, 2), (300, 500, 2), (300, 300, cus // 2 + 2)]
    for Sq, Skv, H in shapes:
        W = H * 128
        q, kv = rand(g, Sq, W), rand(g, Skv, 2 * W)
        for variant in (0, 1, 2, 3):
            def f(q=q, kv=kv, Sq=Sq, W=W, H=H, variant=variant):
                buf, o = out2(Sq, W)
                with Variant(variant):
                    hip.attention_fp8(q, kv[:, :W], kv[:, W:], o, H)
                return [buf]
            cases.append((f"fp8/variant{variant}/Sq{Sq}_Skv{Skv}_H{H}", f))
    S, H = 300, 2
    W = H * 128
    raw = (torch.randn(S, 3 * W, generator=g) * torch.linspace(0.1, 4.0, 3 * W)[None, :]).bfloat16().cuda()
    ids = (torch.arange(S)[:, None] * torch.tensor([0.0, 1.0, 3.0])).float().contiguous().cuda()
    cos, sin = hip.flux_rope_table(ids)
    w = [(1.0 + 0.2 * torch.randn(128, generator=g)).bfloat16().cuda() for _ in range(4)]

    def fused_rope():
        buf, o = out2(S, W)
        hip.attention_fp8_qk_rope(raw, o, H, cos, sin, split=40, wqA=w[0], wkA=w[1], wqB=w[2], wkB=w[3])
        return [buf]
    cases.append(("fp8/fused_qk_norm_rope_S300_H2_split40", fused_rope))
    q, kv = rand(g, S, W), rand(g, S, 2 * W)
    planes = q8_planes(g, S, W)

    def int8_out():
        q8, inv, amax = (t.clone() for t in planes)
        hip.attention_fp8_q8(q, kv[:, :W], kv[:, W:], q8[:S, :W], inv, amax[:S], H)
        return [q8, amax]
    cases.append(("fp8/int8_out_S300_H2", int8_out))
    return cases


def engine_cases():
    def flux_history():
        """ref_in / ref_out: three denoise steps of the tiny FLUX model on the e4m3 attention, steps 2 and 3 starting from the references of the step before."""
        from oracle import flux_ref as R
        from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig, effective_scalar
        cfg = R.tiny_config(num_layers=1, num_single_layers=1)
        m = FluxTransformer2DModel(FluxTransformerConfig(num_layers=1, num_single_layers=1, num_attention_heads=cfg.num_attention_heads,
                                                         joint_attention_dim=cfg.joint_attention_dim, pooled_projection_dim=cfg.pooled_projection_dim),
                                   max_img_tokens=512, max_txt_tokens=64, max_steps=4)
        m.load_state_dict(R.init_weights(cfg, seed=12))
        g = torch.Generator().manual_seed(13)
        h2, w2, T, n = 16, 16, 44, 3                      # S = 300
        lat = torch.randn(h2 * w2, 64, generator=g).bfloat16().cuda()
        pe = torch.randn(T, cfg.joint_attention_dim, generator=g).bfloat16().cuda()
        pool = torch.randn(cfg.pooled_projection_dim, generator=g).bfloat16().cuda()
        sig = R.make_sigmas(n, h2 * w2)
        m.set_condition(pe, pool, R.latent_image_ids(h2, w2))
        m.set_timesteps([effective_scalar(float(s) * 1000.0, torch.bfloat16) for s in sig[:-1]], 3500.0)
        m.set_attention("fp8")
        x = lat.contiguous()
        m.denoise(x, sig)
        torch.cuda.synchronize()
        return [x]

    def qwen2_kv_lens():
        """kv_lens through td_attn_launch: a greedy batched decode of the tiny Qwen2 model, prompts of 17 and 33 tokens.  Sq = 1: the launch chain routes it
        to the decode kernel, not to the tile kernel."""
        from oracle import qwen2vl_ref as R
        from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine, SamplingParams
        cfg = R.tiny_config()
        e = Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                                                num_key_value_heads=cfg.num_kv_heads, intermediate_size=cfg.intermediate, vocab_size=cfg.vocab,
                                                tie_word_embeddings=cfg.tie_embeddings), max_model_len=128, n_slots=8, prefill_rows=300)
        e.load_state_dict(R.init_weights(cfg, seed=23))
        g = torch.Generator().manual_seed(11)
        reqs = [{"prompt_token_ids": torch.randint(0, cfg.vocab, (n,), generator=g).tolist()} for n in (17, 33)]
        res = e.generate_batch(reqs, SamplingParams(temperature=0.0, max_tokens=4, min_tokens=4))
        return [torch.tensor([int(t) for r in res for t in r["token_ids"]], dtype=torch.int32)] + [r["hidden_states"] for r in res]
    return [("engine/flux_tiny_3_steps_fp8_history_references_final_latent", flux_history), ("engine/qwen2_tiny_batched_decode_17_33_launch_chain_to_decode_kernel", qwen2_kv_lens)]


def run_digests(path):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {}
    for name, fn in plain_grid_cases(cus) + streamk_cases(cus) + fp8_cases(cus) + engine_cases():
        bufs = fn()
        torch.cuda.synchronize()
        assert name not in res, name
        res[name] = sha(*bufs)
    with open(path, "w") as fh:      # (one line per launch)
        fh.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(res[k])}" for k in sorted(res)) + "\n}\n")
    print(f"wrote {len(res)} entries to {path} (cus = {cus})")


def compare(a, b):
    A, Bv = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(A) | set(Bv) if A.get(k) != Bv.get(k))
    for k in diff:
        print("differs:", k)
    print(f"{len(diff)} of {len(set(A) | set(Bv))} entries differ between {a} and {b}")
    return 1 if diff else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    assert torch.cuda.is_available(), "attention_digest.py runs the kernels on the MI355X; there is no CPU path"
    if a.out:
        run_digests(a.out)


if __name__ == "__main__":
    main()
