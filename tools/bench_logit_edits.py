"""The logit-edit form of the per-request sampler (td_sample_rows_edit_bf16) and the logprobs kernel (td_logprobs_rows_bf16) beside the paths they
extend, measured in one process at vocab 152 064 with the method of tools/bench_sampler.py.

per launch  us per launch at 1 / 64 / 256 rows of distinct N(0, 3) bf16 logits, temperature 0.6, each case a window of `--launches` launches between
            a hipEvent pair, the cases alternated over `--rounds` rounds, the median reported:
              a    sample_rows, top_k 50 + top_p 0.9                                       (the path that must not get slower)
              p    sample_top_p, top_p 0.9                                                 (likewise)
              b    sample_rows_edit with a NULL edit state                                 (a, through the new entry)
              c    a + a 300-entry bias table and 32 bans per row, every row its own edit slot
              d    a + allow_only of 1000 ids per row
              e0 / e5 / e20   logprobs_rows with n_top = 0, 5, 20 for every row
            a and p are each measured TWICE per round (a, a2; p, p2): the difference of the two medians is the same-build spread.  With
            `--parent-lib PATH` (a libthinkdiff_hip.so built from the parent commit) the parent's td_sample_rows_bf16 / td_sample_top_p_bf16 are
            called through ctypes on the same tensors in the same rounds (a_parent, p_parent): "nothing got slower" means each sits within the spread.
decode step ms per KV-cached decode step of the 7B shape (synthetic weights, 256 sequences, 428 cached tokens), no sampler: c, d and e are reported as a
            share of it, as DESIGN.md 5.14 does.

    python tools/bench_logit_edits.py [--out profiles/logit_edits_bench.json] [--parent-lib PATH] [--launches 50] [--rounds 5] [--no-step]
"""
import argparse
import ctypes
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
T, TOP_P, TOP_K = 0.6, 0.9, 50
N_BIAS, N_BAN, N_ALLOW = 300, 32, 1000


def median(v):
    return sorted(v)[len(v) // 2]


def window_us(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def parent_entries(path):
    """td_sample_rows_bf16 / td_sample_top_p_bf16 of another build of the library, loaded beside this one."""
    L = ctypes.CDLL(path)
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    L.td_sample_rows_bf16.argtypes = [vp, vp, i64, i32, i32, vp, vp, i32, vp, vp]
    L.td_sample_top_p_bf16.argtypes = [vp, i64, i32, i32, f32, f32, ctypes.c_uint64, ctypes.c_uint64, vp, vp]
    L.td_abi_version.restype = ctypes.c_int
    return L


def per_launch(rows, edits, parent, launches, rounds):
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = (torch.randn(rows, VOCAB, generator=g, device="cuda") * 3).bfloat16()
    tab = _hip.pack_sample_rows([dict(temperature=T, top_p=TOP_P, top_k=TOP_K, seed=11, stream=r) for r in range(rows)]).cuda()
    offs = [torch.full((rows,), i, dtype=torch.int64, device="cuda") for i in range(launches)]
    out = torch.empty(rows, dtype=torch.int32, device="cuda")
    cpu = torch.Generator().manual_seed(rows)
    for s in range(rows):                                  # slots [0, rows): bias + bans; slots [256, 256 + rows): allow_only
        perm = torch.randperm(VOCAB, generator=cpu)
        edits.reset_slot(s)
        edits.set_bias(s, {int(t): float(v) for t, v in zip(perm[:N_BIAS].tolist(), (torch.rand(N_BIAS, generator=cpu) * 4 - 2).tolist())})
        edits.ban(s, perm[N_BIAS:N_BIAS + N_BAN].tolist())
        edits.reset_slot(256 + s)
        edits.allow_only(256 + s, perm[:N_ALLOW].tolist())
    slots_c = torch.arange(rows, dtype=torch.int32, device="cuda")
    slots_d = slots_c + 256
    ids = torch.randint(0, VOCAB, (rows,), generator=g, device="cuda", dtype=torch.int32)
    n_top = {n: torch.full((rows,), n, dtype=torch.int32, device="cuda") for n in (0, 5, 20)}
    lp_out = (torch.empty(rows, device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda"),
              torch.empty(rows, 20, dtype=torch.int32, device="cuda"), torch.empty(rows, 20, device="cuda"))
    st = _hip.stream_ptr()
    a_fn = lambda i: _hip.sample_rows(x, tab, offs[i], None, False, out=out)      # noqa: E731
    p_fn = lambda i: _hip.sample_top_p(x, T, TOP_P, 11, i, out=out)               # noqa: E731
    cases = {"a": a_fn, "a2": a_fn, "p": p_fn, "p2": p_fn,
             "b": lambda i: _hip.sample_rows_edit(x, tab, offs[i], None, False, None, None, out=out),
             "c": lambda i: _hip.sample_rows_edit(x, tab, offs[i], None, False, edits, slots_c, out=out),
             "d": lambda i: _hip.sample_rows_edit(x, tab, offs[i], None, False, edits, slots_d, out=out),
             "e0": lambda i: _hip.logprobs_rows(x, ids, n_top[0], 20, out=lp_out),
             "e5": lambda i: _hip.logprobs_rows(x, ids, n_top[5], 20, out=lp_out),
             "e20": lambda i: _hip.logprobs_rows(x, ids, n_top[20], 20, out=lp_out)}
    if parent is not None:
        cases["a_parent"] = lambda i: _hip.check(parent.td_sample_rows_bf16(None, _hip.ptr(x), x.stride(0), rows, VOCAB, _hip.ptr(tab), _hip.ptr(offs[i]), 0, _hip.ptr(out), st))
        cases["p_parent"] = lambda i: _hip.check(parent.td_sample_top_p_bf16(_hip.ptr(x), x.stride(0), rows, VOCAB, T, TOP_P, 11, i, _hip.ptr(out), st))
    for fn in cases.values():                      # warm-up: code objects, allocator
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    same = bool(torch.equal(_hip.sample_rows(x, tab, offs[3]), _hip.sample_rows_edit(x, tab, offs[3], None, False, edits, -1)))
    res = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            res[k].append(window_us(fn, launches))
    rec = {"rows": rows, "edit_form_without_edits_equals_a_bit_for_bit": same, **{f"us_{k}": median(v) for k, v in res.items()},
           **{f"us_{k}_all": v for k, v in res.items()}}
    rec["same_build_spread_us"] = {"a": abs(rec["us_a"] - rec["us_a2"]), "p": abs(rec["us_p"] - rec["us_p2"])}
    if parent is not None:
        rec["this_minus_parent_us"] = {"a": min(rec["us_a"], rec["us_a2"]) - rec["us_a_parent"], "p": min(rec["us_p"], rec["us_p2"]) - rec["us_p_parent"]}
    return rec


def decode_step(steps, rounds):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    B, cached = 256, 428
    e = Qwen2VLTextEngine(Qwen2VLTextConfig(), max_model_len=512, n_slots=B).init_random(1, std=0.02)
    toks = torch.full((B,), 5, dtype=torch.int32, device="cuda")
    pos = [torch.full((3, B), cached + i, dtype=torch.int32, device="cuda") for i in range(32)]

    def run():
        t0 = time.perf_counter()
        for i in range(steps):
            e.decode_batch(toks, pos[i % 32], [cached + i % 32] * B)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    run()
    ms = [run() for _ in range(rounds)]
    del e
    return {"shape": "7B", "sequences": B, "cached_tokens": cached, "steps_per_window": steps, "step_ms_no_sampler": median(ms), "step_ms_no_sampler_all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_edits_bench.json"))
    ap.add_argument("--parent-lib", default=None, help="libthinkdiff_hip.so built from the parent commit, measured beside this build on cases a and p")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logit_edits.py measures on the MI355X; no GPU found")
    parent = parent_entries(a.parent_lib) if a.parent_lib else None
    edits = _hip.logit_edits_create(512, VOCAB)
    rec = {"device": torch.cuda.get_device_name(0), "vocab": VOCAB, "temperature": T, "top_p": TOP_P, "top_k": TOP_K, "launches_per_window": a.launches,
           "rounds": a.rounds, "edits": {"bias_entries": N_BIAS, "bans": N_BAN, "allow_only_ids": N_ALLOW},
           "edit_state_bytes_256_slots": 256 * (2 * ((VOCAB // 8 + 3) // 4 * 4) + 8 * _hip.MAX_LOGIT_BIAS + 4),
           "parent_lib_abi": parent.td_abi_version() if parent is not None else "not measured",
           "note": "us = median over the alternated rounds of (window of launches between two device events) / launches; a: td_sample_rows_bf16 top_k 50 + "
                   "top_p 0.9, p: td_sample_top_p_bf16, a2 / p2: the same again (same-build spread), a_parent / p_parent: the parent commit's library in the same "
                   "rounds, b: td_sample_rows_edit_bf16 with e NULL, c: 300 biases + 32 bans per row, d: allow_only of 1000 ids, e0 / e5 / e20: "
                   "td_logprobs_rows_bf16 with n_top 0 / 5 / 20",
           "per_launch": [per_launch(r, edits, parent, a.launches, a.rounds) for r in ROWS]}
    edits.close()
    if a.no_step:
        rec["decode_step"] = "not measured"
    else:
        st = decode_step(a.steps, a.rounds)
        r256 = next(c for c in rec["per_launch"] if c["rows"] == 256)
        st["share_of_step"] = {k: r256[f"us_{k}"] * 1e-3 / st["step_ms_no_sampler"] for k in ("a", "c", "d", "e0", "e5", "e20")}
        st["extra_over_a_share_of_step"] = {k: (r256[f"us_{k}"] - r256["us_a"]) * 1e-3 / st["step_ms_no_sampler"] for k in ("c", "d")}
        rec["decode_step"] = st
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k != "note"}, indent=1))


if __name__ == "__main__":
    main()
