"""What the decode entries of Qwen2VLTextEngine return, as digests: the record behind a refactor of their host code (profiles/decode_loop_refactor.md).

--out FILE.json   runs a fixed list of generate / generate_batch / generate_continuous / beam_search calls on the tiny model of the GPU tests
                  (oracle.qwen2vl_ref.tiny_config(), init_weights(seed=23), max_model_len 128, 8 slots), on the bf16 and the e4m3 cache, with
                  prefill_rows 300 and with the passes cut at 96 rows (a batch then needs two packed passes, and a 100-token prompt fits none), every
                  call under a freshly seeded generator.  Per call it writes the sha256 of the token ids, of the bytes of prompt_hidden_states and
                  hidden_states (of every output where there are several) and of the logprob values.
--compare A B     lists the entries in which two such files differ; exit status 1 if there are any.
--time            generate_continuous on the 2B shape (synthetic weights): 512 requests of 300 prompt tokens against max_live = 256, 64 tokens each;
                  tokens/s of `--rounds` runs after one untimed run, and their median, as one JSON line.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "thinkdiff-mlre_amd")):
    sys.path.insert(0, p)
from thinkdiff.models.qwen2_vl import BeamSearchParams, Qwen2VLTextConfig, Qwen2VLTextEngine, SamplingParams  # noqa: E402


def sha(data) -> str:
    return hashlib.sha256(data if isinstance(data, bytes) else repr(data).encode()).hexdigest()[:24]


def tensor_sha(t) -> str:
    return sha(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())


def digest(res):
    """One call's results -> four digests over all its requests, in order: the token ids, the bytes of prompt_hidden_states, the bytes of
    hidden_states and the logprob values (cumulative logprobs, scores and per-token logprobs, exact), each of the request's own keys and then of
    every output where there are several."""
    toks, prompt, hidden, scores = [], [], [], []
    for r in (res if isinstance(res, list) else [res]):
        prompt.append(tensor_sha(r["prompt_hidden_states"]))
        for o in [r] + list(r.get("outputs", [])):
            toks.append([int(t) for t in o["token_ids"]])
            hidden.append(tensor_sha(o["hidden_states"]))
            scores.append([float(o[k]).hex() if k in o else None for k in ("cumulative_logprob", "score")] +
                          [[sorted((int(t), float(v.logprob).hex(), int(v.rank)) for t, v in step.items()) for step in o["logprobs"]] if "logprobs" in o else None])
    return {"token_ids": sha(toks), "prompt_hidden_states": sha(prompt), "hidden_states": sha(hidden), "logprobs": sha(scores), "n_tokens": sum(len(t) for t in toks)}


def tiny_engine(kv):
    from oracle import qwen2vl_ref as R
    cfg = R.tiny_config()
    e = Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                                            num_key_value_heads=cfg.num_kv_heads, intermediate_size=cfg.intermediate, vocab_size=cfg.vocab,
                                            tie_word_embeddings=cfg.tie_embeddings), max_model_len=128, n_slots=8, prefill_rows=300, kv_cache_dtype=kv)
    e.load_state_dict(R.init_weights(cfg, seed=23))
    return e, cfg.vocab


def call_list(e, V):
    """(name, fn(generator) -> results).  Prompts of 1 .. 90 tokens, 12 requests, at most 12 generated tokens."""
    g = torch.Generator().manual_seed(11)
    lens = [1, 90, 17, 33, 64, 8, 2, 71, 45, 5, 88, 26]
    reqs = [{"prompt_token_ids": torch.randint(0, V, (n,), generator=g).tolist()} for n in lens]
    six, p0 = reqs[:6], reqs[2]["prompt_token_ids"]
    long_req = {"prompt_token_ids": torch.randint(0, V, (100,), generator=g).tolist()}      # fits no pass of 96 rows
    full_req = {"prompt_token_ids": torch.randint(0, V, (120,), generator=g).tolist()}      # its slot of 128 rows is full after 8 tokens
    greedy = e.generate(p0, SamplingParams(temperature=0.0, max_tokens=6, min_tokens=6))["token_ids"]      # what the stop rules are aimed at
    first = [e.generate(r["prompt_token_ids"], SamplingParams(temperature=0.0, max_tokens=3, min_tokens=3))["token_ids"] for r in reqs]
    forced6 = [[(17 * i + j) % V for j in range(i)] for i in range(6)]
    forced12 = [[(17 * i + j) % V for j in range((2 * i) % 5)] for i in range(12)]
    SP = SamplingParams
    out = []

    def add(name, fn):
        out.append((name, fn))

    add("generate_top_p", lambda gen: e.generate(p0, SP(max_tokens=12, min_tokens=12), generator=gen))
    add("generate_rows_seed_penalty", lambda gen: e.generate(p0, SP(temperature=1.0, seed=3, repetition_penalty=1.2, top_k=50, max_tokens=12, min_tokens=1), generator=gen))
    add("generate_forced_short", lambda gen: e.generate(p0, SP(max_tokens=8, min_tokens=8), forced_output_ids=[5, 6, 7], generator=gen))
    add("generate_forced_long", lambda gen: e.generate(p0, SP(max_tokens=4, min_tokens=4, logprobs=2), forced_output_ids=[5, 6, 7, 8, 9, 10], generator=gen))
    add("generate_logprobs", lambda gen: e.generate(p0, SP(max_tokens=6, min_tokens=6, logprobs=1), generator=gen))
    add("generate_stop_around_min_tokens", lambda gen: e.generate(p0, SP(temperature=0.0, max_tokens=6, min_tokens=2, stop_token_ids=[greedy[0], greedy[3]]), generator=gen))
    add("generate_eos", lambda gen: e.generate(p0, SP(temperature=0.0, max_tokens=6, min_tokens=1, ignore_eos=False), eos_token_id=greedy[2], generator=gen))
    add("generate_n3", lambda gen: e.generate(p0, SP(temperature=1.0, seed=11, n=3, max_tokens=8, min_tokens=1), generator=gen))

    def batch(packed, *a, **kw):
        def run(gen):
            e.packed_prefill = packed
            try:
                return e.generate_batch(*a, generator=gen, **kw)
            finally:
                e.packed_prefill = True
        return run
    for packed in (True, False):
        tag = "packed" if packed else "unpacked"
        add(f"batch_{tag}_top_p_eos_stops", batch(packed, six, SP(temperature=0.0, max_tokens=12, min_tokens=2, ignore_eos=False,
                                                                  stop_token_ids=[first[1][2], first[3][1]]), eos_token_id=first[0][2]))
        add(f"batch_{tag}_sampled", batch(packed, reqs[:8], SP(max_tokens=12, min_tokens=12)))
        add(f"batch_{tag}_long_prompt", batch(packed, [reqs[1], long_req, reqs[5]], SP(max_tokens=6, min_tokens=6)))
    add("batch_list_seeds_budgets_logprobs", batch(True, six, [SP(temperature=1.0, seed=7 * i if i % 2 else None, max_tokens=i % 5, min_tokens=1,
                                                                   logprobs=1 if i % 3 == 0 else None) for i in range(6)]))
    add("batch_forced", batch(True, six, SP(max_tokens=3, min_tokens=3, logprobs=0), forced_output_ids=forced6))
    add("batch_mixed_n_best_of", batch(True, six, [SP(temperature=1.0, seed=30 + i if i != 4 else None, max_tokens=6 + i % 3, min_tokens=1, n=(1, 2, 1, 1, 1, 1)[i],
                                                       best_of=2 if i == 3 else None) for i in range(6)]))
    add("batch_bad_words_and_bias", batch(True, six, [SP(temperature=0.0, max_tokens=6, min_tokens=6, bad_words_token_ids=[first[0][:2]] if i == 0 else None,
                                                          logit_bias={5: 100.0} if i == 1 else None) for i in range(6)]))
    add("batch_reaches_slot_len", batch(True, [full_req, reqs[5], reqs[4]], SP(max_tokens=12, min_tokens=12)))

    add("continuous_top_p_stops", lambda gen: e.generate_continuous(reqs, SP(temperature=0.0, max_tokens=12, min_tokens=2, ignore_eos=False,
                                                                             stop_token_ids=[first[1][2], first[7][1], first[9][2]]),
                                                                    eos_token_id=first[4][2], generator=gen, max_live=4, admit_min=1))
    add("continuous_sampled", lambda gen: e.generate_continuous(reqs, SP(max_tokens=12, min_tokens=12), generator=gen))
    add("continuous_rows_chunks", lambda gen: e.generate_continuous(iter([reqs[:5], reqs[5:]]), [
        SP(temperature=1.0, seed=40 + i if i % 3 else None, max_tokens=3 + i % 4, min_tokens=1, logprobs=0 if i % 4 == 0 else None) for i in range(12)],
        generator=gen, max_live=3, admit_min=2))
    add("continuous_mixed_n_chunks", lambda gen: e.generate_continuous(iter([reqs[:4], reqs[4:9], reqs[9:]]), [
        SP(temperature=1.0, seed=20 + i if i % 4 else None, max_tokens=6 + i % 3, min_tokens=1, n=(1, 3, 2)[i % 3] if i % 4 != 3 else 1,
           best_of=2 if i % 4 == 3 else None) for i in range(12)], generator=gen, max_live=4, admit_min=2))
    add("continuous_forced_with_empty", lambda gen: e.generate_continuous(reqs, SP(max_tokens=13, min_tokens=13), forced_output_ids=forced12, generator=gen,
                                                                          max_live=3, admit_min=1))
    add("continuous_best_of_3", lambda gen: e.generate_continuous(reqs, SP(temperature=1.0, seed=9, n=1, best_of=3, max_tokens=8, min_tokens=1), generator=gen,
                                                                  max_live=7, admit_min=1))
    add("continuous_list_logprobs", lambda gen: e.generate_continuous(reqs, [
        SP(temperature=0.0 if i % 4 == 0 else 1.0, logprobs=i % 3 if i % 2 else None, max_tokens=6 + i % 4, min_tokens=1, ignore_eos=bool(i % 3),
           stop_token_ids=[first[i][1]] if i % 4 == 0 else None) for i in range(12)], eos_token_id=first[3][0], generator=gen, max_live=5, admit_min=2))

    add("beam_r3_w2_eos", lambda gen: e.beam_search([reqs[2], reqs[1], reqs[0]], BeamSearchParams(beam_width=2, max_tokens=8), eos_token_id=greedy[1]))
    add("beam_r1_w3_ignore_eos", lambda gen: e.beam_search([reqs[3]], BeamSearchParams(beam_width=3, max_tokens=12, ignore_eos=True), eos_token_id=greedy[1]))
    add("beam_long_prompt", lambda gen: e.beam_search([reqs[5], long_req], BeamSearchParams(beam_width=2, max_tokens=6, ignore_eos=True)))
    return out


def run_digests(path):
    res = {}
    for kv in ("auto", "fp8"):
        e, V = tiny_engine(kv)
        for rows in (300, 96):
            e.prefill_rows = rows      # (where the host cuts the prefill passes; the workspace keeps its 300 rows)
            for k, (name, fn) in enumerate(call_list(e, V)):
                res[f"{kv}/prefill_rows={rows}/{name}"] = digest(fn(torch.Generator().manual_seed(1000 + k)))
        del e
    with open(path, "w") as fh:      # (one line per call)
        fh.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(res[k])}" for k in sorted(res)) + "\n}\n")
    print(f"wrote {len(res)} entries to {path}")


def compare(a, b):
    A, Bv = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(A) | set(Bv) if A.get(k) != Bv.get(k))
    for k in diff:
        print("differs:", k)
    print(f"{len(diff)} of {len(set(A) | set(Bv))} entries differ between {a} and {b}")
    return 1 if diff else 0


def run_time(rounds, n_req=512, prompt_len=300, max_live=256, new_tokens=64):
    cfg = Qwen2VLTextConfig(hidden_size=1536, num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                            vocab_size=151936, tie_word_embeddings=True)
    e = Qwen2VLTextEngine(cfg, max_model_len=512, n_slots=max_live, prefill_rows=16384).init_random(0)
    g = torch.Generator().manual_seed(5)
    reqs = [{"prompt_token_ids": torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g).tolist()} for _ in range(n_req)]
    sp = SamplingParams(temperature=1.0, top_p=0.95, max_tokens=new_tokens, min_tokens=new_tokens)
    tps = []
    for i in range(rounds + 1):      # (the first run is untimed: step graphs of every batch size the call meets)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = e.generate_continuous(reqs, sp, generator=torch.Generator().manual_seed(7), max_live=max_live)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert sum(len(o["token_ids"]) for o in out) == n_req * new_tokens
        if i:
            tps.append(n_req * new_tokens / dt)
    print(json.dumps({"generate_continuous_tokens_per_s": sorted(tps)[len(tps) // 2], "all": tps, "requests": n_req, "prompt_tokens": prompt_len,
                      "max_live": max_live, "new_tokens": new_tokens, "shape": "2B"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    assert torch.cuda.is_available(), "qwen2_entries_digest.py runs the engine on the MI355X; there is no CPU path"
    if a.time:
        run_time(a.rounds)
    if a.out:
        run_digests(a.out)


if __name__ == "__main__":
    main()
