"""The grouped int4 (AWQ / GPTQ) weight stream of the Qwen2-VL decode engine (td_qwen2_load_param_int4, TD_QWEN2_WEIGHTS_INT4), measured as
tools/bench_qwen2_w4.py measures the MXFP4 one -- in one process, per shape (2B and 7B shapes) one int4 handle loaded from synthetic AWQ tensors and
one mxfp4 handle:

speed    ms per KV-cached decode step for 1 .. 64 sequences in these forms: "bf16" = the int4 handle with its stream off (the bf16 kernels on the SAME
         W^: the yardstick); "int4_all" = the same handle with the stream on and EVERY row count sent to the int4 forms (td_qwen2_set_int4_routing(1)):
         the measurement the engine's routing table is drawn from; "int4" = the stream on with the engine's own routing, what a user gets; "mxfp4" /
         "mxfp4_off" = the mxfp4 handle with its stream on / off.  The forms are timed in rounds that alternate BOTH run orders; a bucket counts as
         faster on int4 (`int4_all_faster_in_both_orders`) only if int4_all beats bf16 in the rounds of either order, and `engine_routes_int4` says
         whether the engine's table sends that bucket to the int4 forms (read off the launch counter): the two columns must agree, and the tool says
         so where they do not.  `generate` for config 3's request (103 prompt + 128 generated tokens) in the same forms.
parent   where profiles/qwen2_mxfp4_bench.json (measured on the parent commit by tools/bench_qwen2_w4.py) has the bucket: the mxfp4 handle's "off" and "on"
         there beside this run's mxfp4 handle's, which must agree within the run-to-run spread.

No quality figures: the synthetic nibbles approximate no trained weights (quality on a trained checkpoint is out of scope; the numerics are tested).

    python tools/bench_qwen2_int4.py [2B] [7B] [--out profiles/qwen2_int4_bench.json] [--steps 100] [--rounds 4] [--group-size 128]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_qwen2_w8 as W8  # noqa: E402  (the shapes and the timed window are the e4m3 bench's)
from bench_qwen2_w8 import N_GEN, N_PROMPT, ROOT, SHAPES, Qwen2VLTextEngine, SamplingParams, linear_elems, time_steps  # noqa: E402

BATCHES = [1, 2, 4, 8, 16, 32, 64]


def synthetic_awq_layer(cfg, layer, G, gen):
    """One decoder layer's seven Linears as AutoAWQ "GEMM" tensors, made on the device: uniform random nibbles and zero points, scales such that the
    dequantised weights have a standard deviation near 0.02."""
    D, I, QW, KVW = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
    extents = {"self_attn.q_proj": (QW, D), "self_attn.k_proj": (KVW, D), "self_attn.v_proj": (KVW, D), "self_attn.o_proj": (D, QW),
               "mlp.gate_proj": (I, D), "mlp.up_proj": (I, D), "mlp.down_proj": (D, I)}

    def words(*shape):      # all 32 bits random
        return (torch.randint(0, 2 ** 32, shape, generator=gen, device="cuda") - 2 ** 31).to(torch.int32)

    sd = {}
    for lin, (N, K) in extents.items():
        base = f"model.layers.{layer}.{lin}"
        sd[base + ".qweight"] = words(K, N // 8)
        sd[base + ".qzeros"] = words(K // G, N // 8)
        sd[base + ".scales"] = ((torch.rand(K // G, N, generator=gen, device="cuda") + 0.5) * (0.02 / 6.5)).half()      # (q - z has a deviation of about 6.5)
    return sd


def int4_handle(cfg, G):
    e = Qwen2VLTextEngine(cfg, max_model_len=512, n_slots=max(BATCHES) + 1, prefill_rows=1024).init_random(0)      # embeddings, norms, biases, lm_head
    e.int4_config = {"quant_method": "awq", "bits": 4, "group_size": G, "version": "gemm", "zero_point": True}
    gen = torch.Generator(device="cuda").manual_seed(7)
    for layer in range(cfg.num_hidden_layers):      # a layer at a time: the checkpoint tensors of the whole model need not sit beside the engine
        e.load_state_dict(synthetic_awq_layer(cfg, layer, G, gen), strict=False)
    return e


def bench_shape(name, cfg, steps, rounds, G, parent):
    elems = linear_elems(cfg) - cfg.vocab_size * cfg.hidden_size      # the decoder Linears: lm_head stays bf16 in an AWQ / GPTQ checkpoint
    out = {"shape": name, "group_size": G, "decoder_linear_bytes_bf16": 2 * elems, "decoder_linear_bytes_int4": elems // 2 + 3 * elems // G,
           "decoder_linear_bytes_mxfp4": elems // 2 + elems // 32, "lm_head_bytes_bf16": 2 * cfg.vocab_size * cfg.hidden_size}
    e4 = int4_handle(cfg, G)
    out["weight_info"] = e4.weight_info()
    assert out["weight_info"]["mode"] == "int4" and out["weight_info"]["bytes_8bit"] == out["decoder_linear_bytes_int4"]
    emx = Qwen2VLTextEngine(cfg, max_model_len=512, n_slots=max(BATCHES) + 1, prefill_rows=1024).init_random(0).quantize_weights("mxfp4")

    def run(key, fn):
        if key == "bf16":
            e4.set_weight_stream(False)
        elif key in ("int4", "int4_all"):
            e4.set_weight_stream(True)
            e4.set_int4_routing(key == "int4_all")
        elif key == "mxfp4_off":
            emx.set_weight_stream(False)
        else:
            emx.set_weight_stream(True)
        return fn(emx if key.startswith("mxfp4") else e4)

    orders = (("bf16", "mxfp4_off", "mxfp4", "int4", "int4_all"), ("int4_all", "int4", "mxfp4", "mxfp4_off", "bf16"))
    par = {r["B"]: r for s in (parent or {}).get("shapes", []) if s["shape"] == name for r in s["decode"]}
    rows = []
    for B in BATCHES:
        ms = {k: {"fwd": [], "rev": []} for k in orders[0]}
        n0 = e4.weight_stream_launches()
        run("int4", lambda e: time_steps(e, B, 2))
        routed = e4.weight_stream_launches() > n0    # the engine's own routing sends this bucket to the int4 forms
        for r in range(rounds):                      # rounds alternate the two run orders
            tag = "rev" if r % 2 else "fwd"
            for key in orders[r % 2]:
                ms[key][tag].append(run(key, lambda e: time_steps(e, B, steps)))
        med = {k: {t: sorted(v[t])[len(v[t]) // 2] for t in v} for k, v in ms.items()}
        allv = {k: v["fwd"] + v["rev"] for k, v in ms.items()}
        row = {"B": B, **{"ms_" + k: sorted(allv[k])[len(allv[k]) // 2] for k in allv}, **{"ms_" + k + "_by_order": med[k] for k in med},
               **{"rounds_" + k: ms[k] for k in ms}, **{"spread_" + k: max(allv[k]) - min(allv[k]) for k in allv}}
        row["int4_all_faster_in_both_orders"] = all(med["int4_all"][t] < med["bf16"][t] for t in ("fwd", "rev"))
        row["engine_routes_int4"] = routed
        row["speedup_int4_all_vs_bf16"] = row["ms_bf16"] / row["ms_int4_all"]
        row["speedup_int4_vs_bf16"] = row["ms_bf16"] / row["ms_int4"]
        row["speedup_int4_all_vs_mxfp4"] = row["ms_mxfp4"] / row["ms_int4_all"]
        if B in par:
            row["parent_mxfp4_handle"] = {"ms_off": par[B]["ms_off"], "ms_on": par[B]["ms_on"], "spread_off": par[B]["spread_off"], "spread_on": par[B]["spread_on"]}
        rows.append(row)
        print(f"{name} decode B={B:3d}: bf16 {row['ms_bf16']:7.3f} (+-{row['spread_bf16']:.3f})  int4_all {row['ms_int4_all']:7.3f} (+-{row['spread_int4_all']:.3f})  "
              f"int4 {row['ms_int4']:7.3f}  mxfp4 {row['ms_mxfp4']:7.3f} (+-{row['spread_mxfp4']:.3f})  mxfp4 off {row['ms_mxfp4_off']:7.3f} ms   int4_all x"
              f"{row['speedup_int4_all_vs_bf16']:5.2f} vs bf16 (faster in both orders: {row['int4_all_faster_in_both_orders']}; engine routes: {routed})"
              + ("" if routed == row["int4_all_faster_in_both_orders"] else "   <-- THE ENGINE'S TABLE DISAGREES WITH THIS MEASUREMENT")
              + (f"   parent mxfp4 off / on {par[B]['ms_off']:.3f} / {par[B]['ms_on']:.3f}" if B in par else ""), flush=True)
    out["decode"] = rows

    # `generate` for one request of config 3: prefill of 103 tokens + 128 KV-cached steps (teacher-forced, so every run does the same work)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, cfg.vocab_size, (N_PROMPT + N_GEN,), generator=g).to(torch.int32)
    sp = SamplingParams(max_tokens=N_GEN, min_tokens=N_GEN, ignore_eos=True)
    ge = {k: [] for k in ("bf16", "mxfp4", "int4", "int4_all")}

    def gen_once(e):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.generate(ids[:N_PROMPT].tolist(), sp, forced_output_ids=ids[N_PROMPT:].tolist())
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for r in range(rounds + 1):
        for key in (tuple(ge) if r % 2 == 0 else tuple(reversed(tuple(ge)))):
            t = run(key, gen_once)
            if r:                                    # round 0 warms every form up
                ge[key].append(t)
    out["generate_103_128_s"] = {**{k: sorted(v)[len(v) // 2] for k, v in ge.items()}, **{"rounds_" + k: v for k, v in ge.items()}}
    print(f"{name} generate 103 + 128 tokens: " + "  ".join(f"{k} {out['generate_103_128_s'][k]:.4f} s" for k in ge), flush=True)
    del e4, emx
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["2B", "7B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen2_int4_bench.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--parent", default=os.path.join(ROOT, "profiles", "qwen2_mxfp4_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qwen2_int4.py measures on the MI355X; there is no CPU path"
    parent = json.load(open(a.parent)) if os.path.exists(a.parent) else None
    res = {"device": torch.cuda.get_device_name(0), "cache_tokens": W8.CACHE, "steps_per_window": a.steps, "rounds": a.rounds,
           "note": "ms = median over the rounds, which alternate the run orders (bf16, mxfp4_off, mxfp4, int4, int4_all) and its reverse; *_by_order = median per "
                   "order; spread = max - min over all rounds; bf16 = the bf16 kernels on the int4 handle's W^ (stream off); int4_all = every row count on the int4 "
                   "forms (td_qwen2_set_int4_routing(1)); int4 = the engine's own routing (engine_routes_int4: whether this bucket reads the int4 copy then; "
                   "where it does not, int4 is the bf16 kernels again); mxfp4 / mxfp4_off = an mxfp4 handle of the "
                   "same shape, stream on / off; parent_mxfp4_handle = that handle's figures in profiles/qwen2_mxfp4_bench.json (the parent commit); synthetic "
                   "AWQ tensors, uniform nibbles",
           "shapes": [bench_shape(n, SHAPES[n], a.steps, a.rounds, a.group_size, parent) for n in a.shapes]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
