"""The KV fork behind n / best_of parallel sampling (td_qwen2_fork_slot, csrc/kv_fork.hip), measured in one process against what it replaces.

copy     per decoder shape (2B, 7B), cache dtype (bf16, e4m3), prompt rows {300, 2048, 8192} and destinations {1, 3, 7}: us per fork of one slot's
         rows to the destinations -- ONE td_qwen2_fork_slot call -- against the loop of td_qwen2_move_slot calls (one per destination: layers x
         planes hipMemcpyAsync each).  A window is `reps` forks between two device events after one untimed fork; the two forms alternate for
         `rounds` rounds; the median is reported with every round's figure, and `spread` = the largest (max - min) / median any form showed in
         the cell (what a difference has to exceed to mean anything).  bytes_moved counts reads and writes: (1 + n_dst) x bytes for the fork
         (the source is loaded once), 2 x n_dst x bytes for the loop; rate_fraction = bytes_moved / time over the copy rate of the box,
         measured in the same process as read + written bytes per second of one 1 GiB device-to-device hipMemcpyAsync.  The weights are left
         unset and the cache holds whatever the allocation held: a copy has no data-dependent path.
generate tokens/s of generate_batch on the 2B shape (synthetic weights): 16 requests of 300 prompt tokens with n = 4 -- 16 prefills, 16 forks --
         against the same 64 sequences submitted as 64 requests (64 prefills), 64 tokens each, alternated, median of `rounds`.

    python tools/bench_kv_fork.py [2B] [7B] [--out profiles/kv_fork_bench.json] [--reps 5] [--rounds 5] [--no-generate]
"""
import argparse
import ctypes
import dataclasses
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thinkdiff-mlre_amd"))
from thinkdiff import _hip  # noqa: E402
from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine, SamplingParams  # noqa: E402

SHAPES = {"2B": Qwen2VLTextConfig(hidden_size=1536, num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                                  vocab_size=151936, tie_word_embeddings=True),
          "7B": Qwen2VLTextConfig()}
ROWS = [300, 2048, 8192]
DSTS = [1, 3, 7]
SLOT_LEN = 8192


def median(v):
    return sorted(v)[len(v) // 2]


def window_us(fn, reps):
    fn()                                       # untimed: first-use costs, and both forms start from the same cache state
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def hip_runtime():
    """The HIP runtime already in the process (torch's), by its mapped path."""
    with open("/proc/self/maps") as fh:
        paths = {line.split()[-1] for line in fh if "libamdhip64" in line}
    assert paths, "no libamdhip64 mapped"
    return ctypes.CDLL(sorted(paths)[0])


def copy_rate(rounds):
    """Bytes read + written per second by one large device-to-device hipMemcpyAsync."""
    rt = hip_runtime()
    rt.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    n = 1 << 30
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    src.zero_()
    dst.zero_()

    def one():
        rc = rt.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n, 3, _hip.stream_ptr())      # 3 = hipMemcpyDeviceToDevice
        assert rc == 0, rc
    us = [window_us(one, 3) for _ in range(rounds)]
    del src, dst
    torch.cuda.empty_cache()
    return 2 * n / (median(us) * 1e-6), us


def bench_copy(name, cfg, reps, rounds, rate):
    cells = []
    for kv in ("auto", "fp8"):
        e = Qwen2VLTextEngine(cfg, max_model_len=SLOT_LEN, n_slots=8, kv_cache_dtype=kv)      # (weights unset: nothing here runs the model)
        row_bytes = e.kv_cache_info()["bytes_per_row"] * cfg.num_hidden_layers
        for rows in ROWS:
            for n_dst in DSTS:
                dst = list(range(1, 1 + n_dst))

                def fork():
                    e.fork_slot(0, dst, rows)

                def loop():
                    for d in dst:
                        e.move_slot(0, d, rows)

                us = {"fork": [], "move_loop": []}
                for _ in range(rounds):
                    us["fork"].append(window_us(fork, reps))
                    us["move_loop"].append(window_us(loop, reps))
                nbytes = rows * row_bytes
                f, m = median(us["fork"]), median(us["move_loop"])
                cell = {"shape": name, "kv_cache_dtype": kv, "rows": rows, "n_dst": n_dst, "slot_bytes_copied": nbytes,
                        "fork_us": f, "move_loop_us": m, "move_loop_over_fork": m / f,
                        "fork_bytes_moved": (1 + n_dst) * nbytes, "move_loop_bytes_moved": 2 * n_dst * nbytes,
                        "fork_rate_fraction": (1 + n_dst) * nbytes / (f * 1e-6) / rate, "move_loop_rate_fraction": 2 * n_dst * nbytes / (m * 1e-6) / rate,
                        "spread": max((max(v) - min(v)) / median(v) for v in us.values()), "us_all": us,
                        "launches": {"fork": 1, "move_loop_memcpys": n_dst * cfg.num_hidden_layers * (2 if kv == "fp8" else 1)}}
                cells.append(cell)
                print(f"{name} {kv:4s} rows={rows:5d} dst={n_dst}: fork {f:9.1f} us ({cell['fork_rate_fraction']:.2f} of the copy rate)   "
                      f"move loop {m:9.1f} us ({cell['move_loop_rate_fraction']:.2f})   x{m / f:.2f}   spread {cell['spread']:.2f}", flush=True)
        del e
        torch.cuda.empty_cache()
    return cells


def bench_generate(rounds, n_req=16, n=4, prompt_len=300, new_tokens=64):
    cfg = SHAPES["2B"]
    e = Qwen2VLTextEngine(cfg, max_model_len=512, n_slots=n_req * n, prefill_rows=16384).init_random(0)
    g = torch.Generator().manual_seed(5)
    reqs = [{"prompt_token_ids": torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g).tolist()} for _ in range(n_req)]
    sp = SamplingParams(temperature=1.0, top_p=0.95, seed=100, max_tokens=new_tokens, min_tokens=new_tokens)

    def forked():
        return e.generate_batch(reqs, dataclasses.replace(sp, n=n))

    def duplicated():       # the same sequences as requests of their own: request i's copy j carries the seed child j gets
        return e.generate_batch([r for r in reqs for _ in range(n)], [dataclasses.replace(sp, seed=sp.seed + j) for _ in reqs for j in range(n)])

    tps = {"n_forked": [], "duplicated_requests": []}
    for fn in (forked, duplicated):
        fn()                # warm: step graphs of every batch size the call meets
    torch.cuda.synchronize()
    for _ in range(rounds):
        for key, fn in (("n_forked", forked), ("duplicated_requests", duplicated)):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert sum(len(c["token_ids"]) for o in out for c in o.get("outputs", [o])) == n_req * n * new_tokens
            tps[key].append(n_req * n * new_tokens / dt)
    res = {"shape": "2B", "requests": n_req, "n": n, "prompt_tokens": prompt_len, "new_tokens": new_tokens,
           "tokens_per_s_n_forked": median(tps["n_forked"]), "tokens_per_s_duplicated_requests": median(tps["duplicated_requests"]),
           "spread": max((max(v) - min(v)) / median(v) for v in tps.values()), "tokens_per_s_all": tps}
    res["n_forked_over_duplicated"] = res["tokens_per_s_n_forked"] / res["tokens_per_s_duplicated_requests"]
    print(f"generate_batch 16 x n=4: {res['tokens_per_s_n_forked']:.0f} tokens/s, as 64 requests: {res['tokens_per_s_duplicated_requests']:.0f} tokens/s "
          f"(x{res['n_forked_over_duplicated']:.2f}, spread {res['spread']:.2f})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["2B", "7B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_fork_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-generate", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kv_fork.py measures on the MI355X; there is no CPU path"
    rate, rate_us = copy_rate(a.rounds)
    print(f"copy rate (1 GiB hipMemcpyAsync, read + written): {rate / 1e12:.2f} TB/s", flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "rounds": a.rounds,
           "copy_rate_bytes_per_s": rate, "copy_rate_window_us": rate_us,
           "note": "us = median of the alternated rounds; move_loop_over_fork > 1: the fork is faster; spread = largest (max - min) / median of a cell's rounds",
           "cells": [c for n in a.shapes for c in bench_copy(n, SHAPES[n], a.reps, a.rounds, rate)]}
    if not a.no_generate:
        res["generate_batch"] = bench_generate(min(a.rounds, 3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
