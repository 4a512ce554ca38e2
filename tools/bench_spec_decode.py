"""Speculative decoding (td_attention_verify, td_qwen2_verify_batch_slots, the speculative generate loop), measured in one process.

attention  per decoder shape (2B, 7B) and cache dtype (bf16, e4m3): us of td_attention_verify in its two forms -- 1 = one workgroup per row (the
           single-row kernel), 2 = the multi-row kernel -- and under the automatic routing, for t rows per sequence {2, 4, 8}, cache lengths
           {256, 2048, 8192} and {1, 8, 32} sequences.  A window is `reps` launches between two device events after one untimed launch; the forms
           alternate for `rounds` rounds; medians, and `auto_is_fastest` per cell (the automatic form within 3 % of the faster one).
step       per shape and weight mode (bf16, MXFP4 stream): us of the verify step with k guesses per sequence {0, 3, 7} for {1, 4, 16} sequences at
           cache length 300 -- k = 0 IS the plain decode step (td_qwen2_decode_batch_slots) -- and its ratio to the plain step of the same handle.
generate   `generate` of 103 + 128 tokens per shape and weight mode, plain and under a synthetic draft source whose guesses are right with
           probability a in {0, 0.5, 1} (it replays the loop's own converged output and spoils a guess with probability 1 - a), alternated; seconds, the
           loop's statistics, and the break-even per-guess probability by linear interpolation between the measured points.

The weights are random: n-gram acceptance on them says nothing about real text, so the acceptance is SET here, not measured; no trained checkpoint is
at hand.

    python tools/bench_spec_decode.py [2B] [7B] [--out profiles/spec_decode_bench.json] [--reps 20] [--rounds 5] [--only attention|step|generate]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thinkdiff-mlre_amd"))
from thinkdiff import _hip  # noqa: E402
from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine, SamplingParams  # noqa: E402

SHAPES = {"2B": Qwen2VLTextConfig(hidden_size=1536, num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                                  vocab_size=151936, tie_word_embeddings=True),
          "7B": Qwen2VLTextConfig()}
T_ROWS, LENGTHS, SEQS = [2, 4, 8], [256, 2048, 8192], [1, 8, 32]


def median(v):
    return sorted(v)[len(v) // 2]


def window_us(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def bench_attention(name, cfg, reps, rounds):
    Hq, Hkv, cells = cfg.num_attention_heads, cfg.num_key_value_heads, []
    L = _hip.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    for kv8 in (False, True):
        S = max(LENGTHS) + 8
        cache = torch.randn(max(SEQS), S, 2 * Hkv * 128, generator=g, device="cuda").bfloat16()
        if kv8:
            by, sc, _ = _hip.kv_quant_rows_e4m3(cache.reshape(-1, 2 * Hkv * 128), 2 * Hkv)
            by, sc = by.reshape(max(SEQS), S, -1), sc.reshape(max(SEQS), S, -1)
            cache_arg = (by[:, :, :Hkv * 128], by[:, :, Hkv * 128:], sc[:, :, :Hkv], sc[:, :, Hkv:])
        else:
            cache_arg = (cache[:, :, :Hkv * 128], cache[:, :, Hkv * 128:])
        for t in T_ROWS:
            for n in SEQS:
                q = torch.randn(n * t, Hq * 128, generator=g, device="cuda").bfloat16()
                o = torch.empty_like(q)
                row0 = torch.arange(n, dtype=torch.int32, device="cuda") * t
                rows = torch.full((n,), t, dtype=torch.int32, device="cuda")
                slot = torch.arange(n, dtype=torch.int32, device="cuda")
                for length in LENGTHS:
                    len0 = torch.full((n,), length - t + 1, dtype=torch.int32, device="cuda")
                    us = {"row": [], "multi": [], "auto": []}
                    for _ in range(rounds):
                        for key, form in (("row", 1), ("multi", 2), ("auto", 0)):
                            # (the host knows t and the length here, as the engine knows its n_new and cache_pos: td_attention_verify_ex takes both)
                            prev = L.td_attention_verify_set_form(form)
                            try:
                                us[key].append(window_us(lambda: _hip.attention_verify(q, cache_arg, row0, rows, len0, slot, Hq, Hkv, out=o, t_max=t, max_len=length), reps))
                            finally:
                                L.td_attention_verify_set_form(prev)
                    med = {k: median(v) for k, v in us.items()}
                    spread = max((max(v) - min(v)) / median(v) for v in us.values())
                    cell = {"shape": name, "kv_cache_dtype": "fp8" if kv8 else "auto", "t": t, "sequences": n, "cache_len": length, "us": med,
                            "multi_over_row": med["multi"] / med["row"], "auto_over_best": med["auto"] / min(med["row"], med["multi"]),
                            "auto_is_fastest": med["auto"] <= 1.03 * min(med["row"], med["multi"]), "spread": spread, "us_all": us}
                    cells.append(cell)
                    print(f"attention {name} {'e4m3' if kv8 else 'bf16'} t={t} seqs={n:2d} len={length:5d}: row {med['row']:7.1f}  multi {med['multi']:7.1f}  auto {med['auto']:7.1f} us"
                          f"   multi/row {cell['multi_over_row']:.2f}  auto fastest {cell['auto_is_fastest']}", flush=True)
        del cache
        torch.cuda.empty_cache()
    return cells


def _engine(cfg, quant, n_slots, slot_len):
    e = Qwen2VLTextEngine(cfg, max_model_len=slot_len, n_slots=n_slots).init_random(0)
    if quant:
        e.quantize_weights(quant)
    return e


def bench_step(name, cfg, reps, rounds, cache_len=300):
    cells = []
    for quant in (None, "mxfp4"):
        e = _engine(cfg, quant, 16, 512)
        for n in (1, 4, 16):
            slots = list(range(n))
            forms = {}
            for k in (0, 3, 7):
                R = n * (k + 1)
                tok = torch.zeros(R, dtype=torch.int32, device="cuda")
                pos = torch.tensor([[cache_len + j for _ in range(n) for j in range(k + 1)]] * 3, dtype=torch.int32, device="cuda")
                forms[k] = (lambda tok=tok, pos=pos, k=k: e.verify_batch(tok, pos, [cache_len] * n, [k + 1] * n, slots=slots)) if k else \
                    (lambda tok=tok, pos=pos: e.decode_batch(tok, pos, [cache_len] * n, slots=slots))
            for fn in forms.values():      # (the plain step captures its graph on the second call)
                fn(), fn(), fn()
            us = {k: [] for k in forms}
            for _ in range(rounds):
                for k, fn in forms.items():
                    us[k].append(window_us(fn, reps))
            med = {k: median(v) for k, v in us.items()}
            cell = {"shape": name, "weights": quant or "bf16", "sequences": n, "cache_len": cache_len, "us": {f"k{k}": v for k, v in med.items()},
                    "over_plain_step": {f"k{k}": med[k] / med[0] for k in (3, 7)}, "spread": max((max(v) - min(v)) / median(v) for v in us.values())}
            cells.append(cell)
            print(f"step {name} {quant or 'bf16':5s} seqs={n:2d}: plain {med[0]:8.1f} us   k=3 {med[3]:8.1f} (x{med[3] / med[0]:.2f})   k=7 {med[7]:8.1f} (x{med[7] / med[0]:.2f})", flush=True)
        del e
        torch.cuda.empty_cache()
    return cells


def break_even(points, plain):
    """The per-guess probability of being right at which the speculative run costs what the plain run costs: linear interpolation between the
    measured (probability, seconds) points; None when they all lie on one side."""
    pts = sorted(points)
    for (a0, s0), (a1, s1) in zip(pts, pts[1:]):
        if (s0 - plain) * (s1 - plain) <= 0 and s0 != s1:
            return a0 + (a1 - a0) * (s0 - plain) / (s0 - s1)
    return None


class SyntheticDraft:
    """Replays a known continuation and spoils each guess with probability 1 - accept (its own generator: the same guesses every round)."""

    def __init__(self, prompt, output, accept, vocab):
        self.seq, self.accept, self.vocab, self.rng = list(prompt) + list(output), accept, vocab, np.random.default_rng(0)

    def propose(self, token_ids, k):
        n = len(token_ids)
        out = np.array(self.seq[n:n + k], dtype=np.int32)
        bad = self.rng.random(out.size) >= self.accept
        return np.where(bad, (out + 1) % self.vocab, out).astype(np.int32)


def bench_generate(name, cfg, rounds, n_prompt=103, n_new=128):
    cells = []
    for quant in (None, "mxfp4"):
        e = _engine(cfg, quant, 1, 512)
        g = torch.Generator().manual_seed(2)
        prompt = torch.randint(0, cfg.vocab_size, (n_prompt,), generator=g).tolist()
        sp = SamplingParams(temperature=0.0, max_tokens=n_new, min_tokens=n_new)
        # The oracle continuation: what the speculative loop itself emits when every guess is right.  A greedy token of a random decoder flips between
        # two schedules, so the plain run's tokens are not it; replaying a run's own output converges in a few rounds (every step is then the same
        # 8-row pass, and a row's result does not depend on the other rows' content).
        plain_out = e.generate(prompt, sp)["token_ids"]
        for _ in range(6):
            nxt = e.generate(prompt, sp, speculative=SyntheticDraft(prompt, plain_out, 1.0, cfg.vocab_size))["token_ids"]
            same, plain_out = nxt == plain_out, nxt
            if same:
                break
        runs = {"plain": lambda: e.generate(prompt, sp)}
        for a in (0.0, 0.5, 1.0):
            runs[f"accept_{a}"] = lambda a=a: e.generate(prompt, sp, speculative=SyntheticDraft(prompt, plain_out, a, cfg.vocab_size))
        sec, stats = {k: [] for k in runs}, {}
        for fn in runs.values():
            fn()
        for _ in range(rounds):
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                sec[k].append(time.perf_counter() - t0)
                if k != "plain":
                    stats[k] = e.spec_stats()
        med = {k: median(v) for k, v in sec.items()}
        rate = {k: (s["accepted"] / s["drafted"] if s["drafted"] else 0.0) for k, s in stats.items()}      # (guesses behind a wrong one count as drafted)
        even = break_even([(float(k.split("_")[1]), med[k]) for k in stats], med["plain"])
        cell = {"shape": name, "weights": quant or "bf16", "prompt_tokens": n_prompt, "new_tokens": n_new, "seconds": med, "stats": stats, "measured_acceptance": rate,
                "speedup_over_plain": {k: med["plain"] / med[k] for k in stats}, "break_even_acceptance": even,
                "spread": max((max(v) - min(v)) / median(v) for v in sec.values())}
        cells.append(cell)
        print(f"generate {name} {quant or 'bf16':5s}: plain {med['plain']:.3f} s   " + "   ".join(f"{k} {med[k]:.3f} s (x{med['plain'] / med[k]:.2f}, {stats[k]['steps']} steps)"
                                                                                                   for k in stats) + f"   break-even acceptance {even}", flush=True)
        del e
        torch.cuda.empty_cache()
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["2B", "7B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_decode_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["attention", "step", "generate"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spec_decode.py measures on the MI355X; there is no CPU path"
    res = {"device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "rounds": a.rounds,
           "note": "medians of alternated rounds in one process; random weights: the acceptance of the generate section is set by a synthetic draft source, "
                   "n-gram acceptance on random weights says nothing about real text and no trained checkpoint is at hand"}
    for n in a.shapes:
        if a.only in (None, "attention"):
            res.setdefault("attention", []).extend(bench_attention(n, SHAPES[n], a.reps, a.rounds))
        if a.only in (None, "step"):
            res.setdefault("step", []).extend(bench_step(n, SHAPES[n], a.reps, a.rounds))
        if a.only in (None, "generate"):
            res.setdefault("generate", []).extend(bench_generate(n, SHAPES[n], max(3, a.rounds // 2 + 1)))
    if "attention" in res:
        res["auto_fastest_in_every_cell"] = all(c["auto_is_fastest"] for c in res["attention"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
