"""The per-request sampler (td_sample_rows_bf16) beside the sampler it extends (td_sample_top_p_bf16), measured in one process at vocab 152 064.

per launch  us per launch at 1 / 64 / 256 rows of distinct N(0, 3) bf16 logits, temperature 0.6, each case a window of `--launches` launches between
            a hipEvent pair, the cases alternated over `--rounds` rounds, the median reported:
              a  sample_top_p, top_p 0.9                                  (the parent's path)
              b  sample_rows, every new field off, top_p 0.9, slot -1    (the same work through the new kernel)
              c  sample_rows, top_k 50 + top_p 0.9
              d  c + repetition 1.1 / presence 0.5 / frequency 0.5 over a history of a 300-token prompt and 128 generated tokens per row,
                 update_state = 1 (the counts are put back to the 128-token history before every window)
decode step ms per KV-cached decode step of the 7B shape (synthetic weights, 256 sequences, 428 cached tokens) followed by one sampler launch on
            the step's own logits, with (a) and with (d), alternated; (d)'s share = its per-launch time at 256 rows over that step time.  Synthetic
            weights give nearly flat logits, so the per-launch figures above are the ones taken on logits with a realistic spread.

    python tools/bench_sampler.py [--out profiles/sampler_rows_bench.json] [--launches 50] [--rounds 5] [--no-step]
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

VOCAB = 152064
ROWS = [1, 64, 256]
N_PROMPT, N_GEN = 300, 128
T, TOP_P = 0.6, 0.9
PEN = dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.5)


def median(v):
    return sorted(v)[len(v) // 2]


def histories(sampler, rows, g):
    """A 300-token prompt and 128 generated tokens (with repeats, as a sampled continuation has) per slot -> the count tensors to restore from."""
    counts = []
    for s in range(rows):
        sampler.reset_slot(s, torch.randint(0, VOCAB, (N_PROMPT,), generator=g, device="cuda", dtype=torch.int32))
        gen = torch.randint(0, VOCAB // 64, (N_GEN,), generator=g, device="cuda") * 64
        counts.append(torch.bincount(gen, minlength=VOCAB).to(torch.int32))
    return counts


def restore(sampler, counts):
    for s, c in enumerate(counts):
        sampler.set_counts(s, c)


def window_us(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def per_launch(rows, sampler, counts, launches, rounds):
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = (torch.randn(rows, VOCAB, generator=g, device="cuda") * 3).bfloat16()
    base = dict(temperature=T, top_p=TOP_P, seed=11)
    tab = {"b": _hip.pack_sample_rows([dict(base, stream=r) for r in range(rows)]).cuda(),
           "c": _hip.pack_sample_rows([dict(base, stream=r, top_k=50) for r in range(rows)]).cuda(),
           "d": _hip.pack_sample_rows([dict(base, stream=r, top_k=50, slot=r, **PEN) for r in range(rows)]).cuda()}
    offs = [torch.full((rows,), i, dtype=torch.int64, device="cuda") for i in range(launches)]
    out = torch.empty(rows, dtype=torch.int32, device="cuda")
    cases = {"a": lambda i: _hip.sample_top_p(x, T, TOP_P, 11, i, out=out),
             "b": lambda i: _hip.sample_rows(x, tab["b"], offs[i], None, False, out=out),
             "c": lambda i: _hip.sample_rows(x, tab["c"], offs[i], None, False, out=out),
             "d": lambda i: _hip.sample_rows(x, tab["d"], offs[i], sampler, True, out=out)}
    for fn in cases.values():                      # warm-up: code objects, allocator
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    same = bool(torch.equal(_hip.sample_top_p(x, T, TOP_P, 11, 3), _hip.sample_rows(x, tab["b"], offs[3])))
    res = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            if k == "d":
                restore(sampler, counts[:rows])
                torch.cuda.synchronize()
            res[k].append(window_us(fn, launches))
    return {"rows": rows, "b_equals_a_bit_for_bit": same, **{f"us_{k}": median(v) for k, v in res.items()}, **{f"us_{k}_all": v for k, v in res.items()}}


def decode_step(sampler, counts, steps, rounds):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    B, cached = 256, N_PROMPT + N_GEN
    e = Qwen2VLTextEngine(Qwen2VLTextConfig(), max_model_len=512, n_slots=B).init_random(1, std=0.02)
    toks = torch.full((B,), 5, dtype=torch.int32, device="cuda")
    pos = [torch.full((3, B), cached + i, dtype=torch.int32, device="cuda") for i in range(32)]
    tab_d = _hip.pack_sample_rows([dict(temperature=T, top_p=TOP_P, seed=11, stream=r, top_k=50, slot=r, **PEN) for r in range(B)]).cuda()
    offs = [torch.full((B,), i, dtype=torch.int64, device="cuda") for i in range(32)]
    out = torch.empty(B, dtype=torch.int32, device="cuda")

    def step(i, mode):
        _, lg = e.decode_batch(toks, pos[i % 32], [cached + i % 32] * B)
        if mode == "a":
            _hip.sample_top_p(lg, T, TOP_P, 11, i, out=out)
        elif mode == "d":
            _hip.sample_rows(lg, tab_d, offs[i % 32], sampler, True, out=out)

    def run(mode):
        t0 = time.perf_counter()
        for i in range(steps):
            step(i, mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for mode in ("none", "a", "d"):
        for i in range(3):
            step(i, mode)
    torch.cuda.synchronize()
    res = {"none": [], "a": [], "d": []}
    for _ in range(rounds):
        for mode in res:
            if mode == "d":
                restore(sampler, counts)
                torch.cuda.synchronize()
            res[mode].append(run(mode))
    del e
    return {"shape": "7B", "sequences": B, "cached_tokens": cached, "steps_per_window": steps,
            **{f"step_ms_{'no_sampler' if k == 'none' else 'with_' + k}": median(v) for k, v in res.items()},
            **{f"step_ms_{'no_sampler' if k == 'none' else 'with_' + k}_all": v for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_rows_bench.json"))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler.py measures on the MI355X; no GPU found")
    sampler = _hip.sampler_create(256, VOCAB)
    counts = histories(sampler, 256, torch.Generator(device="cuda").manual_seed(0))
    rec = {"device": torch.cuda.get_device_name(0), "vocab": VOCAB, "temperature": T, "top_p": TOP_P, "launches_per_window": a.launches, "rounds": a.rounds,
           "history": {"prompt_tokens": N_PROMPT, "generated_tokens": N_GEN, **PEN},
           "state_bytes": 256 * (VOCAB * 2 + 2 * ((VOCAB // 8 + 3) // 4 * 4)),
           "note": "us = median over the alternated rounds of (window of launches between two device events) / launches; a: td_sample_top_p_bf16, "
                   "b: td_sample_rows_bf16 everything off, c: top_k 50 + top_p 0.9, d: c + three penalties over 300 + 128 history tokens, update_state 1",
           "per_launch": [per_launch(r, sampler, counts, a.launches, a.rounds) for r in ROWS]}
    if not a.no_step:
        st = decode_step(sampler, counts, a.steps, a.rounds)
        d256 = next(c for c in rec["per_launch"] if c["rows"] == 256)["us_d"]
        st["sampler_d_share_of_step"] = d256 * 1e-3 / st["step_ms_with_d"]
        st["sampler_a_share_of_step"] = next(c for c in rec["per_launch"] if c["rows"] == 256)["us_a"] * 1e-3 / st["step_ms_with_a"]
        rec["decode_step"] = st
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k != "note"}, indent=1))


if __name__ == "__main__":
    main()
