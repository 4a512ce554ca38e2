"""The e4m3 KV cache of the Qwen2-VL decode engine (td_qwen2_create_kv, vLLM's kv_cache_dtype="fp8"), measured in one process: per shape (2B, 7B;
synthetic weights) two handles with the same init_random seed -- bf16 cache and e4m3 cache -- alternated.

speed    ms per KV-cached decode step (replayed step graphs, 100 per window closed by a device synchronise, median of 3 windows) for
         sequences {1, 8, 64, 256} x cached tokens {300, 2048, 8192}; a cell is left out where the handle cannot hold it (the 2^31-element row limit
         of td_qwen2_create: 256 sequences x 8192 rows x 1024 elements on the 7B shape).  The cache CONTENTS of the timed steps are whatever the
         handles hold (random bf16 rows / zero bytes): the kernels have no data-dependent path, the figures are bytes moved and instructions issued;
attention  us per launch of the decode attention alone on the same shapes: td_attention_decode_kv8 against the bf16 op (td_attention_bf16 with
         Sq = 1) on a cache holding the same values, each as ONE replayed graph of 20 launches between a hipEvent pair -- eager launches through
         the Python wrappers cost the host ~13 - 20 us each, more than the short kernels take;
memory   both handles' cache_bytes (td_qwen2_kv_info);
quality  a record only, no bar: relative RMSE of the teacher-forced model.norm hidden states (103 prompt rows, 128 decode steps) of the e4m3-cache
         handle against the bf16-cache handle, and top-1 agreement of the logits over the 128 forced steps.  Synthetic N(0, 0.02) weights give
         nearly flat logits and no trained checkpoint is on hand, so these say little about a real model.

    python tools/bench_qwen2_kv8.py [2B] [7B] [--out profiles/qwen2_kv8_bench.json] [--steps 100] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thinkdiff-mlre_amd"))
from thinkdiff import _hip  # noqa: E402
from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine  # noqa: E402

SHAPES = {"2B": Qwen2VLTextConfig(hidden_size=1536, num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                                  vocab_size=151936, tie_word_embeddings=True),
          "7B": Qwen2VLTextConfig()}
SEQS = [1, 8, 64, 256]
CACHED = [300, 2048, 8192]
SLOT_LEN = 8192 + 256             # room for the longest cell and the 32 positions a window walks, also when 64 such slots are re-cut into 256
N_PROMPT, N_GEN = 103, 128


def time_steps(e, B, cached, steps):
    toks = torch.full((B,), 5, dtype=torch.int32, device="cuda")
    pos = [torch.full((3, B), cached + i, dtype=torch.int32, device="cuda") for i in range(32)]      # (device tensors: no copy inside the window)
    for i in range(3):            # eager, captured, replayed: the timed window replays the step graph
        e.decode_batch(toks, pos[i], [cached + i] * B, want_logits=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        e.decode_batch(toks, pos[i % 32], [cached + i % 32] * B, want_logits=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def teacher_forced(e, ids):
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


def median(v):
    return sorted(v)[len(v) // 2]


def attention_us(cfg, B, skv, rounds, launches=20):
    """us per launch of the decode attention alone: the bf16 op and the e4m3 op on caches holding the same values K^ | V^, alternated.  Each op's
    `launches` launches are captured into one graph once; a timed window is one replay of it, so no host work sits between the kernels."""
    Hq, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    KVW = 2 * Hkv * 128
    g = torch.Generator(device="cuda").manual_seed(B * 7 + skv)
    q = torch.randn(B, 1, Hq * 128, generator=g, device="cuda", dtype=torch.bfloat16)
    kv = torch.randn(B * skv, KVW, generator=g, device="cuda", dtype=torch.bfloat16)
    q8, sc, _ = _hip.kv_quant_rows_e4m3(kv, 2 * Hkv, inplace=True)          # kv now holds the values the bytes hold
    kv3, q83, sc3 = kv.view(B, skv, KVW), q8.view(B, skv, KVW), sc.view(B, skv, 2 * Hkv)
    out = torch.empty(B, 1, Hq * 128, dtype=torch.bfloat16, device="cuda")
    lens = torch.full((B,), skv, dtype=torch.int32, device="cuda")

    def bf16():
        _hip.attention(q, kv3[:, :, :Hkv * 128], kv3[:, :, Hkv * 128:], out, Hq, Hkv, causal=True)

    def kv8():
        _hip.attention_decode_kv8(q[:, 0], q83[:, :, :Hkv * 128], q83[:, :, Hkv * 128:], sc3[:, :, :Hkv], sc3[:, :, Hkv:], Hq, Hkv, kv_lens=lens, out=out[:, 0])

    graphs = {}
    for name, fn in (("bf16", bf16), ("e4m3", kv8)):
        fn()                          # (eager once: one-time attributes are set outside a capture)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(launches):
                fn()
    us = {"bf16": [], "e4m3": []}
    for _ in range(rounds):
        for name in ("bf16", "e4m3"):
            graphs[name].replay()     # warm
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graphs[name].replay()
            b.record()
            b.synchronize()
            us[name].append(a.elapsed_time(b) / launches * 1e3)
    del graphs, kv, q8, sc
    torch.cuda.empty_cache()
    return median(us["bf16"]), median(us["e4m3"]), us


def bench_shape(name, cfg, steps, rounds):
    KVW = 2 * cfg.num_key_value_heads * 128
    # the most slots whose SLOT_LEN rows pass the engine's 2^31-element limit on a layer's cache (and 256 at the most)
    n_slots = max(s for s in SEQS if s * SLOT_LEN * KVW < (1 << 31))
    out = {"shape": name, "slots_at_full_length": n_slots, "slot_len": SLOT_LEN}
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, cfg.vocab_size, (N_PROMPT + N_GEN,), generator=g).to(torch.int32)
    eng = {kv: Qwen2VLTextEngine(cfg, max_model_len=SLOT_LEN, n_slots=n_slots, kv_cache_dtype=kv).init_random(0) for kv in ("auto", "fp8")}
    out["kv_cache_info"] = {kv: e.kv_cache_info() for kv, e in eng.items()}
    out["cache_bytes_ratio"] = out["kv_cache_info"]["fp8"]["cache_bytes"] / out["kv_cache_info"]["auto"]["cache_bytes"]
    print(f"{name}: {out['kv_cache_info']}", flush=True)

    h16, top16 = teacher_forced(eng["auto"], ids)
    h8, top8 = teacher_forced(eng["fp8"], ids)
    out["quality"] = {"hidden_rel_rmse_prompt_e4m3_vs_bf16_cache": rel_rmse(h8[:N_PROMPT], h16[:N_PROMPT]),
                      "hidden_rel_rmse_decode_e4m3_vs_bf16_cache": rel_rmse(h8[N_PROMPT:], h16[N_PROMPT:]),
                      "top1_agreement_e4m3_vs_bf16_cache": sum(a == b for a, b in zip(top8, top16)) / N_GEN, "forced_steps": N_GEN,
                      "for_scale": "fp64 attention over K^ | V^ against K | V on N(0, 1) operands at 300 keys: 3.6e-2 relative RMSE (CPU)"}
    print(f"{name} quality: {out['quality']}", flush=True)

    rows = []
    for B in SEQS:
        if B > n_slots:           # more sequences than fit at full length: re-partition the same rows
            for e in eng.values():
                e.set_slots(B)
        for cached in CACHED:
            row = {"sequences": B, "cached_tokens": cached}
            if cached + 40 <= min(e.slot_len for e in eng.values()):
                ms = {"auto": [], "fp8": []}
                for _ in range(rounds):                  # alternated: bf16 cache, e4m3 cache, ...
                    for kv in ("auto", "fp8"):
                        ms[kv].append(time_steps(eng[kv], B, cached, steps))
                row.update(step_ms_bf16=median(ms["auto"]), step_ms_e4m3=median(ms["fp8"]), step_ms_bf16_all=ms["auto"], step_ms_e4m3_all=ms["fp8"])
                row["step_ratio_bf16_over_e4m3"] = row["step_ms_bf16"] / row["step_ms_e4m3"]
            else:
                row["step_not_measured"] = f"{B} sequences x {cached} rows x {KVW} elements exceed the engine's 2^31-element limit on a layer's cache"
            a16, a8, all_us = attention_us(cfg, B, cached, rounds)
            row.update(attn_us_bf16=a16, attn_us_e4m3=a8, attn_ratio_bf16_over_e4m3=a16 / a8, attn_us_all=all_us)
            rows.append(row)
            print(f"{name} B={B:3d} cached={cached:5d}: step " + (f"{row['step_ms_bf16']:8.3f} -> {row['step_ms_e4m3']:8.3f} ms (x{row['step_ratio_bf16_over_e4m3']:.2f})"
                  if "step_ms_bf16" in row else "   (not held)") + f"   attention {a16:8.1f} -> {a8:8.1f} us (x{a16 / a8:.2f})", flush=True)
    out["cells"] = rows
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["2B", "7B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen2_kv8_bench.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qwen2_kv8.py measures on the MI355X; there is no CPU path"
    res = {"device": torch.cuda.get_device_name(0), "steps_per_window": a.steps, "rounds": a.rounds,
           "note": "ms / us = median of the alternated rounds; ratio > 1: the e4m3 cache is faster; synthetic N(0, 0.02) weights; quality is a record, not a bar",
           "shapes": [bench_shape(n, SHAPES[n], a.steps, a.rounds) for n in a.shapes]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
