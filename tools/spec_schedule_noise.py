"""How far two EXISTING schedules of one tiny decoder sit from each other, per Linear init: what sizes the models of tests/test_spec_decode_gpu.py.

For the two decoder widths (hidden 1536 with 12 / 2 heads, hidden 3584 with 28 / 4; 2 layers, MLP 2048, vocabulary 2048), weight seeds 7, 8, 9 and the
Linear std either the oracle's flat 0.02 or 0.02 sqrt(512 / hidden) (the layer gain of the project's tiny config): `generate` one request at a time
against `generate_batch` on the same forced ids -- the pair tests/test_qwen2_gpu.py::test_batched_decode_equals_one_sequence_at_a_time compares under
_rel < 5e-3 -- and prints the largest rel-RMS difference of the hidden states, the largest difference of one token's logprob (top 5 of every position)
and the positions where the two disagree on the best token.  None of the speculative code runs.

    python tools/spec_schedule_noise.py [--out profiles/spec_schedule_noise.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thinkdiff-mlre_amd"))
sys.path.insert(0, ROOT)
from oracle import qwen2vl_ref as Q  # noqa: E402
from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine, SamplingParams  # noqa: E402

SHAPES = {"1536": dict(hidden_size=1536, num_attention_heads=12, num_key_value_heads=2), "3584": dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4)}
VOCAB = 2048


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def requests():
    g = torch.Generator().manual_seed(17)
    out = []
    for n in (12, 30, 7, 21):
        ids = torch.randint(0, VOCAB, (n,), generator=g).tolist()
        out.append({"prompt_token_ids": ids + ids[:5]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_schedule_noise.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "spec_schedule_noise.py measures on the MI355X"
    cells = []
    for scaled in (False, True):
        for seed in (7, 8, 9):
            for name, d in SHAPES.items():
                std = 0.02 * (512 / d["hidden_size"]) ** 0.5 if scaled else 0.02
                oc = Q.tiny_config(hidden=d["hidden_size"], num_heads=d["num_attention_heads"], num_kv_heads=d["num_key_value_heads"], intermediate=2048, vocab=VOCAB)
                e = Qwen2VLTextEngine(Qwen2VLTextConfig(num_hidden_layers=2, intermediate_size=2048, vocab_size=VOCAB, **d), max_model_len=1024)
                e.load_state_dict(Q.init_weights(oc, seed=seed, std=std))
                e.set_slots(8)
                reqs = requests()
                forced = [r["token_ids"] for r in e.generate_batch(reqs, SamplingParams(temperature=0.0, max_tokens=24, min_tokens=24))]
                sp = SamplingParams(max_tokens=24, min_tokens=24, logprobs=5)
                single = [e.generate(r["prompt_token_ids"], sp, forced_output_ids=f) for r, f in zip(reqs, forced)]
                single = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()} for o in single]
                batch = e.generate_batch(reqs, sp, forced_output_ids=forced)
                worst, flips, hid = 0.0, 0, 0.0
                for x, y in zip(single, batch):
                    hid = max(hid, rel(x["hidden_states"], y["hidden_states"]))
                    for dx, dy in zip(x["logprobs"], y["logprobs"]):
                        worst = max([worst] + [abs(dx[t].logprob - dy[t].logprob) for t in set(dx) & set(dy)])
                        flips += max(dx, key=lambda t: dx[t].logprob) != max(dy, key=lambda t: dy[t].logprob)
                cells.append({"hidden": int(name), "weight_seed": seed, "linear_std": std, "scaled": scaled, "hidden_rel": hid, "max_dlogprob": worst,
                              "best_token_disagreements_of_96": flips})
                print(f"hidden {name} seed {seed} std {std:.4f}: hidden rel {hid:.2e}  max |d logprob| {worst:.5f}  best-token disagreements {flips} of 96", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "note": "generate one request at a time against generate_batch on the same forced ids; no "
                   "speculative code runs", "cells": cells}, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
