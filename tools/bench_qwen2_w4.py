"""The MXFP4 weight stream of the Qwen2-VL decode engine (td_qwen2_quantize_weights, TD_QWEN2_WEIGHTS_MXFP4), measured as tools/bench_qwen2_w8.py
measures the e4m3 one -- in one process, one mxfp4 handle per shape (2B and 7B shapes, synthetic weights):

speed    ms per KV-cached decode step with the stream off and on, alternated on the SAME mxfp4 handle (the model is the same either way; "off" is
         the bf16 kernels on W^), for 1 .. 64 sequences and 65 as the control that reads bf16 either way, and in the same rounds an fp8 handle of
         the same shape with its stream on (the e4m3 column); `generate` for config 3's request (103 prompt + 128 generated tokens);
quality  an unquantised handle with the same weights W against the mxfp4 one (weights W^): relative RMSE of the teacher-forced model.norm hidden
         states and top-1 agreement of the logits over the 128 forced steps, and stream on against off.  Synthetic N(0, 0.02) weights give nearly
         flat logits, so the top-1 figure is a pessimistic stand-in for a trained checkpoint.

    python tools/bench_qwen2_w4.py [2B] [7B] [--out profiles/qwen2_mxfp4_bench.json] [--steps 100] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_qwen2_w8 as W8  # noqa: E402  (the shapes, the timed window and the teacher-forced run are the e4m3 bench's)
from bench_qwen2_w8 import BATCHES, N_GEN, N_PROMPT, ROOT, SHAPES, Qwen2VLTextEngine, SamplingParams, linear_elems, rel_rmse, teacher_forced, time_steps  # noqa: E402


def bench_shape(name, cfg, steps, rounds):
    elems = linear_elems(cfg)
    out = {"shape": name, "linear_weight_bytes_bf16": 2 * elems, "linear_weight_bytes_e4m3": elems, "linear_weight_bytes_mxfp4": elems // 2 + elems // 32}
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, cfg.vocab_size, (N_PROMPT + N_GEN,), generator=g).to(torch.int32)

    def handle(quantization=None):
        e = Qwen2VLTextEngine(cfg, max_model_len=512, n_slots=max(BATCHES) + 1, prefill_rows=1024).init_random(0)
        return e.quantize_weights(quantization) if quantization else e

    ref = handle()                                   # the unquantised model, weights W
    h_ref, top_ref = teacher_forced(ref, ids)
    del ref
    torch.cuda.empty_cache()

    e = handle("mxfp4")
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

    e8 = handle("fp8")                               # the e4m3 column: another model (its own W^), the same launches
    rows = []
    for B in BATCHES:
        ms = {"off": [], "on": [], "e4m3": []}
        for _ in range(rounds):                      # alternated: off, on, e4m3, off, on, e4m3, ...
            for key in ms:
                if key != "e4m3":
                    e.set_weight_stream(key == "on")
                ms[key].append(time_steps(e8 if key == "e4m3" else e, B, steps))
        med = {k: sorted(v)[rounds // 2] for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        by4 = out["linear_weight_bytes_mxfp4"] if B <= 64 else out["linear_weight_bytes_bf16"]
        rows.append({"B": B, "ms_off": med["off"], "ms_on": med["on"], "ms_e4m3": med["e4m3"], "ms_off_all": ms["off"], "ms_on_all": ms["on"],
                     "ms_e4m3_all": ms["e4m3"], "spread_off": spread["off"], "spread_on": spread["on"], "spread_e4m3": spread["e4m3"],
                     "speedup_vs_off": med["off"] / med["on"], "speedup_vs_e4m3": med["e4m3"] / med["on"],
                     "weight_TBps_off": out["linear_weight_bytes_bf16"] / med["off"] / 1e9, "weight_TBps_on": by4 / med["on"] / 1e9})
        print(f"{name} decode B={B:3d}: off {med['off']:7.3f} (+-{spread['off']:.3f})  on {med['on']:7.3f} (+-{spread['on']:.3f})  e4m3 {med['e4m3']:7.3f} "
              f"(+-{spread['e4m3']:.3f}) ms   x{med['off'] / med['on']:5.2f} vs off, x{med['e4m3'] / med['on']:5.2f} vs e4m3", flush=True)
    out["decode"] = rows

    # `generate` for one request of config 3: prefill of 103 tokens + 128 KV-cached steps (teacher-forced, so every run does the same work)
    sp = SamplingParams(max_tokens=N_GEN, min_tokens=N_GEN, ignore_eos=True)
    ge = {"off": [], "on": [], "e4m3": []}
    for r in range(rounds + 1):
        for key in ge:
            if key != "e4m3":
                e.set_weight_stream(key == "on")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (e8 if key == "e4m3" else e).generate(ids[:N_PROMPT].tolist(), sp, forced_output_ids=ids[N_PROMPT:].tolist())
            torch.cuda.synchronize()
            if r:                                    # round 0 warms every form up
                ge[key].append(time.perf_counter() - t0)
    out["generate_103_128_s"] = {**{k: sorted(v)[rounds // 2] for k, v in ge.items()}, **{k + "_all": v for k, v in ge.items()}}
    print(f"{name} generate 103 + 128 tokens: " + "  ".join(f"{k} {out['generate_103_128_s'][k]:.4f} s" for k in ge), flush=True)
    del e, e8
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["2B", "7B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen2_mxfp4_bench.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qwen2_w4.py measures on the MI355X; there is no CPU path"
    res = {"device": torch.cuda.get_device_name(0), "cache_tokens": W8.CACHE, "steps_per_window": a.steps, "rounds": a.rounds,
           "note": "ms = median of the alternated rounds, spread = max - min of the rounds; off = bf16 kernels on the mxfp4 handle's W^; e4m3 = an fp8 "
                   "handle of the same shape, stream on; synthetic N(0, 0.02) weights; pixel RMSE of config 3 with quantisation on: not measured",
           "shapes": [bench_shape(n, SHAPES[n], a.steps, a.rounds) for n in a.shapes]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
