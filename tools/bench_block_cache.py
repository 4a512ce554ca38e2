"""The first-block cache at 1024 x 1024, 28 steps, T = 512 on a full-size synthetic FLUX.1-dev transformer, one and two images in flight, in one
process: one JSON object with
  * rates[in_flight][config] -- images/s of the engine's own loop (td_flux_denoise / td_flux_denoise_multi) with the cache off and under the fixed
                                schedules that skip about 0, 1/4, 1/2 and 3/4 of steps 1 .. 27 (evenly spread; `skipped` holds the counts), the
                                configurations alternated round by round; `vs_off` is each rate over the cache-off rate of the same in-flight count
  * threshold                -- threshold mode, FOR INFORMATION ONLY: the synthetic checkpoint's natural skip rate says nothing about real weights
  * skipped_step             -- what one skipped forward costs (host clock around a run of skipped forwards, each with its stream synchronisation),
                                beside the traced kernel time of the same launches with the cache off -- a full-width model of ONE double block and
                                no single block: x_embedder, block 0, the final norm and proj_out are its whole forward -- and of one full forward
For the two kernels alone: `python tools/bench_ops.py blockcache`.

    python tools/bench_block_cache.py [--size 1024] [--steps 28] [--rounds 2] [--warmup 1] [--txt 512] [--threshold 0.1] [--out profiles/block_cache_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "thinkdiff-mlre_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def spread_schedule(n: int, fraction: float):
    """compute[i] for n forwards: step 0 computed, about `fraction` of steps 1 .. n - 1 skipped, evenly spread."""
    return [1] + [0 if int(i * fraction) != int((i - 1) * fraction) else 1 for i in range(1, n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--txt", type=int, default=512)
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    from thinkdiff.models import FirstBlockCacheConfig
    from thinkdiff.models.flux_prompt import FlowMatchEulerSchedule, FluxPipelineRewritePrompt
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig, effective_scalar

    torch.cuda.set_device(0)
    S, T, N = a.size, a.txt, a.steps
    n_tok = (S // 16) ** 2
    caps = dict(max_img_tokens=n_tok, max_txt_tokens=T, max_steps=max(32, N))
    pipe = FluxPipelineRewritePrompt.from_random(seed=1234, with_vae=False, **caps)
    ctxs, tr = pipe._contexts(2), pipe.transformer
    streams = pipe._streams[:2]
    g = torch.Generator().manual_seed(0)
    pe = torch.randn(2, T, 4096, generator=g).bfloat16().cuda()
    pooled = torch.randn(2, 768, generator=g).bfloat16().cuda()
    lat0 = torch.randn(2, n_tok, 64, generator=g).bfloat16().cuda()
    ids = FluxPipelineRewritePrompt._prepare_latent_image_ids(S // 16, S // 16, "cuda")
    sig = FlowMatchEulerSchedule.sigmas(N, n_tok)
    t_eff = [effective_scalar(float(s) * 1000.0, torch.bfloat16) for s in sig[:-1]]
    g_eff = float((torch.tensor([3.5]).bfloat16() * 1000).float())

    def prepare(m, k):
        m.set_condition(pe[k], pooled[k], ids)
        m.set_timesteps(t_eff, g_eff)

    def run(G):
        """G images through the loop; returns (seconds, latents)."""
        for k in range(G):
            prepare(ctxs[k], k)
        xs = [lat0[k].clone() for k in range(G)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if G == 1:
            tr.denoise(xs[0], sig)
        else:
            FluxTransformer2DModel.denoise_multi(ctxs[:G], xs, sig, streams[:G])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, xs

    fractions = {"skip_0": 0.0, "skip_1_4": 0.25, "skip_1_2": 0.5, "skip_3_4": 0.75}
    schedules = {k: spread_schedule(N, f) for k, f in fractions.items()}

    def configure(name):
        if name == "off":
            tr.disable_cache()
        elif name == "threshold":
            tr.enable_cache(FirstBlockCacheConfig(threshold=a.threshold))
        else:
            tr.set_cache_schedule(schedules[name])

    names = ["off"] + list(schedules) + ["threshold"]
    res = {"metric": "block_cache", "size": S, "txt_tokens": T, "steps": N, "seq": T + n_tok, "precision": "bf16",
           "skipped": {k: N - sum(v) for k, v in schedules.items()}, "rates": {}, "rounds": {}}
    identical = None
    for G in (1, 2):
        secs = {n: [] for n in names}
        outs = {}
        for r in range(a.warmup + a.rounds):
            for n in names:      # alternated: every round visits every configuration
                configure(n)
                dt, xs = run(G)
                if r >= a.warmup:
                    secs[n].append(dt)
                outs[n] = xs
                if n == "threshold":
                    outs["threshold_log"] = [ctxs[k].cache_stats() for k in range(G)]
        rate = {n: round(G * len(v) / sum(v), 4) for n, v in secs.items()}
        res["rates"][str(G)] = {n: {"images_per_s": rate[n], "vs_off": round(rate[n] / rate["off"], 3)} for n in names}
        res["rounds"][str(G)] = {n: [round(G / v, 4) for v in vs] for n, vs in secs.items()}
        if G == 1:      # a schedule without skips changes no bit
            identical = bool(torch.equal(outs["off"][0], outs["skip_0"][0]))
            log = outs["threshold_log"][0]
            res["threshold"] = {"note": "for information only: a synthetic checkpoint's natural skip rate says nothing about real weights", "threshold": a.threshold,
                                "skipped_of_%d" % N: N - sum(log[1]), "decisions": "".join("C" if c else "s" for c in log[1]),
                                "metrics": [None if m == float("inf") else round(m, 4) for m in log[0]]}
    res["skip_0_equals_off_bits"] = identical

    # ---- one skipped forward: host clock (the stream synchronisation of every forward included) vs the parent's traced kernels ----------------
    prepare(tr, 0)
    n_skip = 16
    tr.set_cache_schedule([1] + [0] * n_skip)
    x = lat0[0].clone()
    for rep in range(2):      # first pass warms the skipped path up
        tr.reset_cache()
        tr.forward_step(x, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_skip):
            tr.forward_step(x, 1 + i % (N - 1))
        torch.cuda.synchronize()
        skipped_ms = (time.perf_counter() - t0) * 1e3 / n_skip
    assert tr.cache_stats()[1] == [True] + [False] * n_skip
    tr.disable_cache()

    def traced_ms(m, k):
        m.forward_step(x, 0)
        torch.cuda.synchronize()
        m.trace_begin(1024)
        m.forward_step(x, 1)
        t = m.trace_end()
        return {c: round(v["ms"], 3) for c, v in t.items() if v["launches"]}, sum(v["ms"] for v in t.values()), sum(v["launches"] for v in t.values())

    full = min((traced_ms(tr, 0) for _ in range(2)), key=lambda r: r[1])
    one = FluxTransformer2DModel(FluxTransformerConfig(num_layers=1, num_single_layers=0), **caps).init_random(1234)
    prepare(one, 0)
    head = min((traced_ms(one, 0) for _ in range(3)), key=lambda r: r[1])
    res["skipped_step"] = {"skipped_forward_ms_host_clock": round(skipped_ms, 3),
                           "same_launches_cache_off_traced_ms": round(head[1], 3), "same_launches_count": head[2], "same_launches_by_category_ms": head[0],
                           "ratio": round(skipped_ms / head[1], 3),
                           "full_forward_traced_ms": round(full[1], 3), "full_forward_launches": full[2],
                           "skipped_over_full": round(skipped_ms / full[1], 4)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
