"""The 8-bit weight stream of the Qwen2-VL decode engine (td_qwen2_quantize_weights), measured in one process on one handle per shape (2B and 7B
shapes, synthetic weights):

speed    ms per KV-cached decode step with the stream off and on, alternated on the SAME quantised handle (the model is the same either way), for
         1 .. 64 sequences and 65 as the control that reads bf16 either way; the implied weight bytes per second; get_embed's engine part for
         config 3's token counts (103 prompt + 128 generated tokens, one request);
quality  a second, unquantised handle with the same weights W against the quantised one (weights W^): relative RMSE of the teacher-forced
         model.norm hidden states (103 prompt rows, 128 decode steps) and top-1 agreement of the logits over the 128 forced steps.  Synthetic
         N(0, 0.02) weights give nearly flat logits, so the top-1 figure is a pessimistic stand-in for a trained checkpoint.

    python tools/bench_qwen2_w8.py [2B] [7B] [--out profiles/qwen2_w8_bench.json] [--steps 100] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thinkdiff-mlre_amd"))
from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine, SamplingParams  # noqa: E402

SHAPES = {"2B": Qwen2VLTextConfig(hidden_size=1536, num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                                  vocab_size=151936, tie_word_embeddings=True),
          "7B": Qwen2VLTextConfig()}
BATCHES = [1, 2, 4, 8, 16, 32, 64, 65]
CACHE = 300                       # tokens already cached per sequence while a step is timed
N_PROMPT, N_GEN = 103, 128        # config 3's request: prompt and generated tokens


def linear_elems(cfg):
    """Elements of the Linear weights a decode step streams (every layer's q|k|v, o, gate|up, down and lm_head)."""
    D, I = cfg.hidden_size, cfg.intermediate_size
    return cfg.num_hidden_layers * (D * (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * 128 + cfg.num_attention_heads * 128 * D + 3 * D * I) + cfg.vocab_size * D


def time_steps(e, B, steps):
    toks = torch.full((B,), 5, dtype=torch.int32, device="cuda")
    pos = [torch.full((3, B), CACHE + i, dtype=torch.int32, device="cuda") for i in range(32)]      # (device tensors: no copy inside the window)
    for i in range(3):            # eager, captured, replayed: the timed window replays the step graph
        e.decode_batch(toks, pos[i], [CACHE + i] * B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        e.decode_batch(toks, pos[i % 32], [CACHE + i % 32] * B)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def teacher_forced(e, ids):
    """model.norm hidden states of the prompt rows and of every forced decode step, and the argmax of each step's logits."""
    pos = Qwen2VLTextEngine.text_position_ids(len(ids))
    hid_p, _ = e.forward(pos[:, :N_PROMPT], ids[:N_PROMPT], slot=0)
    hids, tops = [hid_p.float().cpu()], []
    for i in range(N_PROMPT, len(ids)):
        h, lg = e.decode_batch(ids[i:i + 1], pos[:, i:i + 1], [i])
        hids.append(h.float().cpu())
        tops.append(int(lg[0].float().argmax()))
    torch.cuda.synchronize()
    return torch.cat(hids), tops


def rel_rmse(a, b):
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def bench_shape(name, cfg, steps, rounds):
    out = {"shape": name, "linear_weight_bytes_bf16": 2 * linear_elems(cfg), "linear_weight_bytes_8bit": linear_elems(cfg)}
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, cfg.vocab_size, (N_PROMPT + N_GEN,), generator=g).to(torch.int32)

    def handle():
        return Qwen2VLTextEngine(cfg, max_model_len=512, n_slots=max(BATCHES) + 1, prefill_rows=1024).init_random(0)

    ref = handle()                                   # the unquantised model, weights W
    h_ref, top_ref = teacher_forced(ref, ids)
    del ref
    torch.cuda.empty_cache()

    e = handle()
    e.quantize_weights("fp8")
    out["weight_info"] = e.weight_info()
    h_hat, top_hat = teacher_forced(e, ids)
    e.set_weight_stream(False)
    h_off, top_off = teacher_forced(e, ids)
    e.set_weight_stream(True)
    out["quality"] = {
        "hidden_rel_rmse_prompt_vs_unquantised": rel_rmse(h_hat[:N_PROMPT], h_ref[:N_PROMPT]),
        "hidden_rel_rmse_decode_vs_unquantised": rel_rmse(h_hat[N_PROMPT:], h_ref[N_PROMPT:]),
        "top1_agreement_vs_unquantised": sum(a == b for a, b in zip(top_hat, top_ref)) / N_GEN,
        "hidden_rel_rmse_decode_stream_on_vs_off": rel_rmse(h_hat[N_PROMPT:], h_off[N_PROMPT:]),
        "top1_agreement_stream_on_vs_off": sum(a == b for a, b in zip(top_hat, top_off)) / N_GEN,
        "forced_steps": N_GEN,
    }
    print(f"{name} quality: {out['quality']}", flush=True)

    rows = []
    for B in BATCHES:
        ms = {False: [], True: []}
        for _ in range(rounds):                      # alternated: off, on, off, on, ...
            for on in (False, True):
                e.set_weight_stream(on)
                ms[on].append(time_steps(e, B, steps))
        off, on = sorted(ms[False])[rounds // 2], sorted(ms[True])[rounds // 2]
        by8 = out["linear_weight_bytes_8bit"] if B <= 64 else out["linear_weight_bytes_bf16"]
        rows.append({"B": B, "ms_off": off, "ms_on": on, "ms_off_all": ms[False], "ms_on_all": ms[True], "speedup": off / on,
                     "weight_TBps_off": out["linear_weight_bytes_bf16"] / off / 1e9, "weight_TBps_on": by8 / on / 1e9})
        print(f"{name} decode B={B:3d}: off {off:7.3f} ms  on {on:7.3f} ms  x{off / on:5.2f}   weights {rows[-1]['weight_TBps_off']:5.2f} -> {rows[-1]['weight_TBps_on']:5.2f} TB/s", flush=True)
    out["decode"] = rows

    # get_embed's engine part for one request of config 3: prefill of 103 tokens + 128 KV-cached steps (teacher-forced, so both runs do the same work)
    sp = SamplingParams(max_tokens=N_GEN, min_tokens=N_GEN, ignore_eos=True)
    ge = {False: [], True: []}
    for r in range(rounds + 1):
        for on in (False, True):
            e.set_weight_stream(on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.generate(ids[:N_PROMPT].tolist(), sp, forced_output_ids=ids[N_PROMPT:].tolist())
            torch.cuda.synchronize()
            if r:                                    # round 0 warms both forms up
                ge[on].append(time.perf_counter() - t0)
    out["get_embed_103_128_s"] = {"off": sorted(ge[False])[rounds // 2], "on": sorted(ge[True])[rounds // 2], "off_all": ge[False], "on_all": ge[True]}
    print(f"{name} generate 103 + 128 tokens: off {out['get_embed_103_128_s']['off']:.4f} s  on {out['get_embed_103_128_s']['on']:.4f} s", flush=True)
    del e
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["2B", "7B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen2_w8_bench.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qwen2_w8.py measures on the MI355X; there is no CPU path"
    res = {"device": torch.cuda.get_device_name(0), "cache_tokens": CACHE, "steps_per_window": a.steps, "rounds": a.rounds,
           "note": "ms = median of the alternated rounds; synthetic N(0, 0.02) weights; pixel RMSE of config 3 with quantisation on: not measured",
           "shapes": [bench_shape(n, SHAPES[n], a.steps, a.rounds) for n in a.shapes]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
