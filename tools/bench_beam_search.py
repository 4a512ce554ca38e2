"""Beam search on the device (td_beam_select + td_kv_gather_rows, Qwen2VLTextEngine.beam_search), measured in one process.

round    per decoder shape (2B, 7B), cache dtype (bf16, e4m3), beam width W {4, 10}, requests R {1, 16} and cache length {300, 2048, 8192}: us per
         round of  beam_select + gather_slots  on R x W rows, for three outcomes of the choice -- `none` (every beam stays in its row: nothing is
         copied, the cost is the two launches), `half` (the lower-ranked half of each request's beams died and take copies of its best beam's rows)
         and `all_but_one` (only the best beam survived) -- beside the us of the decode step the round belongs to (decode_batch of R x W rows at that
         cache length, synthetic weights) and their ratio.  A window is `reps` rounds between two device events after one untimed round; the forms
         alternate for `rounds` rounds; medians, every round's figure and `spread` = the largest (max - min) / median of the cell.
search   the whole beam_search (R = 16, W = 4, 300 prompt tokens, 64 new tokens, 2B shape) against the host-planned loop it replaces -- per step
         logprobs_rows, ONE download of the candidates, the choice in Python, td_qwen2_fork_slot per parent with several children, decode_batch --
         alternated in one process; seconds per call, medians and spread.  Both return the same beams (checked on the token lists).

    python tools/bench_beam_search.py [2B] [7B] [--out profiles/beam_search_bench.json] [--reps 5] [--rounds 5] [--no-search]
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
from thinkdiff.models.qwen2_vl import BeamSearchParams, Qwen2VLTextConfig, Qwen2VLTextEngine  # noqa: E402

SHAPES = {"2B": Qwen2VLTextConfig(hidden_size=1536, num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                                  vocab_size=151936, tie_word_embeddings=True),
          "7B": Qwen2VLTextConfig()}
WIDTHS, REQUESTS, LENGTHS = [4, 10], [1, 16], [300, 2048, 8192]
SLOT_LEN = 8192 + 8


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


def copy_pattern(R, W, kind):
    """copy_src [R W] as td_beam_select would leave it: `none`; `half`: rows W/2.. of a request copy its row 0; `all_but_one`: rows 1.. do."""
    src = np.full((R, W), -1, dtype=np.int32)
    first = {"none": W, "half": W // 2, "all_but_one": 1}[kind]
    src[:, first:] = (np.arange(R, dtype=np.int32) * W)[:, None]
    return torch.from_numpy(src.reshape(-1)).cuda()


def bench_round(name, cfg, reps, rounds):
    cells = []
    for kv in ("auto", "fp8"):
        e = Qwen2VLTextEngine(cfg, max_model_len=SLOT_LEN, n_slots=max(WIDTHS) * max(REQUESTS), kv_cache_dtype=kv).init_random(0)
        row_bytes = e.kv_cache_info()["bytes_per_row"] * cfg.num_hidden_layers
        g = torch.Generator().manual_seed(1)
        for W in WIDTHS:
            for R in REQUESTS:
                N = R * W
                logits = torch.randn(N, cfg.vocab_size, generator=g).bfloat16().cuda()
                _, _, top_ids, top_lp = _hip.logprobs_rows(logits, [0] * N, 2 * W, 2 * W)
                cum, rank = torch.zeros(N, device="cuda"), torch.arange(W, dtype=torch.int32).repeat(R).cuda()
                out = _hip.beam_select(top_ids, top_lp, cum, rank, W, W, -1)
                slots = list(range(N))
                tok, pos = torch.zeros(N, dtype=torch.int32), None
                for L in LENGTHS:
                    pos = torch.full((3, N), L, dtype=torch.int32)
                    forms = {"decode_step": lambda: e.decode_batch(tok, pos, [L] * N, slots=slots)}
                    for kind in ("none", "half", "all_but_one"):
                        src = copy_pattern(R, W, kind)
                        forms[kind] = lambda src=src: (_hip.beam_select(top_ids, top_lp, cum, rank, W, W, -1, out=out), e.gather_slots(slots, src, [L] * N))
                    us = {k: [] for k in forms}
                    for _ in range(rounds):
                        for k, fn in forms.items():
                            us[k].append(window_us(fn, reps))
                    med = {k: median(v) for k, v in us.items()}
                    cell = {"shape": name, "kv_cache_dtype": kv, "W": W, "R": R, "cache_len": L, "decode_step_us": med["decode_step"],
                            "select_gather_us": {k: med[k] for k in ("none", "half", "all_but_one")},
                            "share_of_decode_step": {k: med[k] / med["decode_step"] for k in ("none", "half", "all_but_one")},
                            "rows_copied": {"none": 0, "half": R * (W - W // 2), "all_but_one": R * (W - 1)}, "bytes_per_copied_row": L * row_bytes,
                            "spread": max((max(v) - min(v)) / median(v) for v in us.values()), "us_all": us}
                    cells.append(cell)
                    print(f"{name} {kv:4s} W={W:2d} R={R:2d} len={L:5d}: decode {med['decode_step']:8.1f} us   select+gather none {med['none']:7.1f}  half {med['half']:8.1f}  "
                          f"all_but_one {med['all_but_one']:8.1f} us   ({med['none'] / med['decode_step']:.3f} / {med['half'] / med['decode_step']:.3f} / "
                          f"{med['all_but_one'] / med['decode_step']:.3f} of the step)   spread {cell['spread']:.2f}", flush=True)
        del e
        torch.cuda.empty_cache()
    return cells


def host_planned(e, prompts, W, T):
    """The loop beam_search replaces, from decode_batch, logprobs_rows and fork_slot: one download and up to W fork launches per request and step.
    -> per request the W token lists by rank."""
    R, plen = len(prompts), [len(p) for p in prompts]
    rows = [e.forward(e.text_position_ids(n), torch.tensor(p, dtype=torch.int32), None, 0, True, True, slot=r * W)[1] for r, (p, n) in enumerate(zip(prompts, plen))]
    logits = torch.stack(rows)
    beams = [[(r * W, [], np.float32(0.0))] for r in range(R)]
    for s in range(T):
        n = logits.shape[0]
        _, _, tid, tlp = _hip.logprobs_rows(logits, [0] * n, 2 * W, 2 * W)
        tid, tlp = tid.cpu().numpy(), tlp.cpu().numpy()
        row, feed = 0, []
        for r in range(R):
            cands = []
            for k, (_, _, cum) in enumerate(beams[r]):
                cands += [(-float(cum + tlp[row, c]), k, c) for c in range(2 * W)]
                row += 1
            cands.sort()
            row0 = row - len(beams[r])
            free = [sl for sl in range(r * W, r * W + W) if sl not in {beams[r][k][0] for _, k, _ in cands[:W]}]
            kids = {}
            for _, k, c in cands[:W]:
                kids.setdefault(k, []).append(c)
            new = {}
            for k, cs in kids.items():
                slot, toks, cum = beams[r][k]
                dst = [free.pop() for _ in cs[1:]]
                if dst:
                    e.fork_slot(slot, dst, plen[r] + s)
                for c, sl in zip(cs, [slot] + dst):
                    new[(k, c)] = (sl, toks + [int(tid[row0 + k, c])], np.float32(cum + tlp[row0 + k, c]))
            beams[r] = [new[(k, c)] for _, k, c in cands[:W]]
            feed += [(b, plen[r] + s) for b in beams[r]]
        _, logits = e.decode_batch([b[1][-1] for b, _ in feed], [[m for _, m in feed]] * 3, [m for _, m in feed], slots=[b[0] for b, _ in feed])
    return [[b[1] for b in bs] for bs in beams]


def bench_search(rounds, R=16, W=4, prompt_len=300, T=64):
    cfg = SHAPES["2B"]
    e = Qwen2VLTextEngine(cfg, max_model_len=512, n_slots=R * W, prefill_rows=16384).init_random(0)
    e.packed_prefill = False      # (both forms prefill one prompt per forward, so that they see the same cache rows)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g).tolist() for _ in range(R)]
    bp = BeamSearchParams(beam_width=W, max_tokens=T, ignore_eos=True)

    def device():
        return [[c["token_ids"] for c in o["outputs"]] for o in e.beam_search([{"prompt_token_ids": p} for p in prompts], bp)]

    def host():
        return host_planned(e, prompts, W, T)

    same = sum(a == b for x, y in zip(device(), host()) for a, b in zip(x, y))
    torch.cuda.synchronize()
    sec = {"device": [], "host_planned": []}
    for _ in range(rounds):
        for key, fn in (("device", device), ("host_planned", host)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            sec[key].append(time.perf_counter() - t0)
    res = {"shape": "2B", "requests": R, "beam_width": W, "prompt_tokens": prompt_len, "new_tokens": T, "equal_beams": same, "beams": R * W,
           "seconds_device": median(sec["device"]), "seconds_host_planned": median(sec["host_planned"]),
           "spread": max((max(v) - min(v)) / median(v) for v in sec.values()), "seconds_all": sec}
    res["host_planned_over_device"] = res["seconds_host_planned"] / res["seconds_device"]
    print(f"beam_search {R} x W={W}, {T} tokens: {res['seconds_device']:.3f} s, host-planned loop {res['seconds_host_planned']:.3f} s "
          f"(x{res['host_planned_over_device']:.2f}, spread {res['spread']:.2f}); {same} of {R * W} beams equal", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["2B", "7B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_search_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-search", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_beam_search.py measures on the MI355X; there is no CPU path"
    res = {"device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "rounds": a.rounds,
           "note": "us = median of the alternated rounds; select_gather_us = td_beam_select + td_qwen2_gather_slots per round for three outcomes of the choice; "
                   "share_of_decode_step = that over the decode step of the same rows and cache length; spread = largest (max - min) / median of a cell's rounds"}
    if not a.no_search:
        res["beam_search"] = bench_search(a.rounds)
    res["cells"] = [c for n in a.shapes for c in bench_round(n, SHAPES[n], a.reps, a.rounds)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
