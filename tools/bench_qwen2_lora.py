"""Per-request LoRA on the Qwen2-VL decode engine (td_qwen2_lora_*, td_lora_rows_bf16), measured in one process per shape (2B and 7B shapes) on ONE
handle with LoRA enabled:

decode   ms per KV-cached decode step at 1, 8, 32, 64 and 256 sequences, at ranks 16 and 64, in four arms: "none" = no row names an adapter (the launch
         list of a handle without LoRA: the yardstick), "one" = one adapter on every row, "four" = four adapters mixed row by row, "half" = one adapter on
         every second row.  The arms alternate inside every round and the table keeps the median and every round's figure (the spread).
prefill  ms of one packed prefill of 1024 rows (8 prompts of 128 tokens) in the same arms.
kernels  the shrink + expand pair alone behind each of the four fused Linears (q|k|v, o, gate|up, down) at the decode row counts, one adapter on every
         row: microseconds per call and the bytes the pair must move, computed from the shapes (x, the adapter's A and B, the fp32 slabs written and read
         back, y read and written).

Synthetic adapters (A, B ~ 0.02 N(0, 1) on all seven Linears of every layer); no quality figures: none is trained.

    python tools/bench_qwen2_lora.py [2B] [7B] [--out profiles/qwen2_lora_bench.json] [--steps 40] [--rounds 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_qwen2_w8 import CACHE, ROOT, SHAPES, Qwen2VLTextEngine, time_steps  # noqa: E402  (the shapes and the timed window are the e4m3 bench's)

from thinkdiff import _hip  # noqa: E402
from thinkdiff.models import qwen2_lora as L  # noqa: E402

BATCHES = [1, 8, 32, 64, 256]
RANKS = [16, 64]
ARMS = ["none", "one", "four", "half"]
PREFILL_PROMPTS, PREFILL_LEN = 8, 128


def synthetic_adapter(cfg, rank, seed):
    """A and B of all seven Linears of every layer, made on the device (the pool's loader takes them from there)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    pairs = {}
    for layer in range(cfg.num_hidden_layers):
        for m, (N, K) in L.module_shapes(cfg).items():
            pairs[(layer, m)] = ((0.02 * torch.randn(rank, K, generator=g, device="cuda")).bfloat16(), (0.02 * torch.randn(N, rank, generator=g, device="cuda")).bfloat16())
    return L.Adapter(rank, 2.0, pairs)


def assignment(arm, rank, n):
    """The LoRARequest (or None) of each of n rows."""
    ids = {r: [L.LoRARequest(f"r{r}-{i}", 100 * r + i) for i in range(1, 5)] for r in RANKS}[rank]
    if arm == "none":
        return [None] * n
    if arm == "one":
        return [ids[0]] * n
    if arm == "four":
        return [ids[i % 4] for i in range(n)]
    return [ids[0] if i % 2 == 0 else None for i in range(n)]


def bind(e, arm, rank, slots):
    e._lora.release_all()
    e._lora.bind(list(slots), assignment(arm, rank, len(slots)))


def median(v):
    return sorted(v)[len(v) // 2]


def pair_bytes(rows, K, widths, rank):
    """Bytes the shrink + expand pair must move for one adapter on every row: x, A and B once, the fp32 slabs out and back, y in and out."""
    rp, rows16 = (rank + 15) // 16 * 16, (rows + 15) // 16 * 16
    slabs = min(32, (K + 255) // 256)
    steps = -(-(K // 32) // slabs)
    slabs = -(-(K // 32) // steps)
    return 2 * rows * K + sum(2 * rp * (K + w) for w in widths) + 2 * 4 * slabs * len(widths) * rows16 * rp + sum(2 * 2 * rows * w for w in widths)


def time_pair(cfg, rows, rank, reps=50):
    D, I, QW, HW = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
    out = {}
    for name, K, widths in (("qkv", D, [QW, HW, HW]), ("o", QW, [D]), ("gate_up", D, [I, I]), ("down", I, [D])):
        x = torch.randn(rows, K, device="cuda").bfloat16()
        ys = [torch.randn(rows, w, device="cuda").bfloat16() for w in widths]
        packed = [[_hip.lora_rows_pack((0.02 * torch.randn(rank, K, device="cuda")).bfloat16(), (0.02 * torch.randn(w, rank, device="cuda")).bfloat16()) for w in widths]]
        ra = torch.zeros(rows, dtype=torch.int32, device="cuda")
        ws = torch.empty(_hip.lora_rows_workspace_bytes(rows, K, len(widths), rank), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            _hip.lora_rows(x, ra, packed, [rank], [2.0], ys, workspace=ws)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            _hip.lora_rows(x, ra, packed, [rank], [2.0], ys, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) / reps * 1e3
        by = pair_bytes(rows, K, widths, rank)
        out[name] = {"us": us, "bytes": by, "GBps": by / us / 1e3}
    return out


def time_prefill(e, reps=5):
    g = torch.Generator().manual_seed(3)
    rows = [{"position_ids": Qwen2VLTextEngine.text_position_ids(PREFILL_LEN), "token_ids": torch.randint(0, 1000, (PREFILL_LEN,), generator=g).tolist()}
            for _ in range(PREFILL_PROMPTS)]
    emb = [dict(position_ids=r["position_ids"], inputs_embeds=e.embed_tokens(r["token_ids"])) for r in rows]
    slots = list(range(PREFILL_PROMPTS))

    def once():
        _hip.check(e._L.td_qwen2_prefill_packed_slots(e._h, PREFILL_PROMPTS, _slots_c, None, _hip.ptr(packed_emb), _hip.ptr(pos), _lens_c, _hip.ptr(hid), None, _hip.stream_ptr()))

    packed_emb = torch.cat([r["inputs_embeds"] for r in emb])
    pos = torch.cat([r["position_ids"] for r in emb], dim=1).to("cuda", torch.int32).contiguous()
    hid = torch.empty_like(packed_emb)
    _slots_c = ctypes.cast((ctypes.c_int * PREFILL_PROMPTS)(*slots), ctypes.c_void_p)
    _lens_c = ctypes.cast((ctypes.c_int * PREFILL_PROMPTS)(*[PREFILL_LEN] * PREFILL_PROMPTS), ctypes.c_void_p)
    once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        once()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def bench_shape(name, cfg, steps, rounds):
    e = Qwen2VLTextEngine(cfg, max_model_len=512, n_slots=max(BATCHES) + 1, prefill_rows=1024, enable_lora=True, max_loras=4, max_lora_rank=max(RANKS)).init_random(0)
    for r in RANKS:
        ad = synthetic_adapter(cfg, r, seed=r)      # (one set of tensors under four ids: the kernels do not care, the host memory does)
        for i in range(1, 5):
            e._lora.register(L.LoRARequest(f"r{r}-{i}", 100 * r + i), ad)
    out = {"shape": name, "lora_info": None, "decode": [], "prefill_1024_rows": [], "kernels": []}
    for B in BATCHES:
        for rank in RANKS:
            ms = {a: [] for a in ARMS}
            for _ in range(rounds):
                for arm in ARMS:
                    bind(e, arm, rank, range(B))
                    ms[arm].append(time_steps(e, B, steps))
            row = {"B": B, "rank": rank, **{f"ms_{a}": median(ms[a]) for a in ARMS}, **{f"ms_{a}_all": ms[a] for a in ARMS}}
            row.update({f"overhead_{a}": median(ms[a]) / median(ms["none"]) - 1 for a in ARMS[1:]})
            out["decode"].append(row)
            print(f"{name} decode B={B:3d} r={rank:2d}: " + "  ".join(f"{a} {row['ms_' + a]:7.3f}" for a in ARMS) + "  ms   overhead " +
                  "  ".join(f"{a} {100 * row['overhead_' + a]:+6.1f} %" for a in ARMS[1:]), flush=True)
        out["kernels"].append({"rows": B, **{f"rank{r}": time_pair(cfg, B, r) for r in RANKS}})
        print(f"{name} kernel pair at {B} rows: " + json.dumps(out["kernels"][-1]), flush=True)
    for rank in RANKS:
        ms = {a: [] for a in ARMS}
        for _ in range(rounds):
            for arm in ARMS:
                e._lora.release_all()
                e._lora.bind(list(range(PREFILL_PROMPTS)), assignment("four" if arm == "four" else arm, rank, PREFILL_PROMPTS))
                ms[arm].append(time_prefill(e))
        row = {"rows": PREFILL_PROMPTS * PREFILL_LEN, "rank": rank, **{f"ms_{a}": median(ms[a]) for a in ARMS}, **{f"ms_{a}_all": ms[a] for a in ARMS}}
        row.update({f"overhead_{a}": median(ms[a]) / median(ms["none"]) - 1 for a in ARMS[1:]})
        out["prefill_1024_rows"].append(row)
        print(f"{name} prefill 1024 rows r={rank:2d}: " + "  ".join(f"{a} {row['ms_' + a]:7.3f}" for a in ARMS) + "  ms", flush=True)
    out["kernels"].append({"rows": 1024, **{f"rank{r}": time_pair(cfg, 1024, r, reps=20) for r in RANKS}})
    out["lora_info"] = e.lora_info()
    del e
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["2B", "7B"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen2_lora_bench.json"))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qwen2_lora.py measures on the MI355X; there is no CPU path"
    res = {"device": torch.cuda.get_device_name(0), "cache_tokens": CACHE, "steps_per_window": a.steps, "rounds": a.rounds,
           "note": "ms = median of the rounds, arms alternated inside every round, *_all = every round; 'none' is the launch list of a handle without LoRA; "
                   "synthetic adapters on all seven Linears of every layer; kernels: one adapter on every row",
           "shapes": [bench_shape(n, SHAPES[n], a.steps, a.rounds) for n in a.shapes]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
