"""FLUX.1 Redux on full-size synthetic weights (random, the released shapes), every figure measured in one process: one JSON line with
  * prior_ms                 -- per image: the SigLIP so400m tower (27 layers, 729 tokens), the two-Linear prior and the composition of the stream
                                (td_redux_compose_bf16 twice: 512 zero text rows + 729 image rows, and the pooled vector), device time between events,
                                with the number of C-ABI calls each part makes (host-composed: the tower is launch-bound)
  * t512_images_per_s        -- text-to-image at 1024 x 1024, 28 steps, a prompt stream of T = 512 rows (a plain T5 prompt)
  * t1241_images_per_s       -- the same loop with T = 1241 rows (512 text + 729 Redux tokens): the per-step cost of Redux is the longer text stream
and the ratio beside the row-count arithmetic (Linears (4096 + 1241) / (4096 + 512) = 1.16 x, joint attention 1.34 x).  The yardstick is the T = 512
rate of THIS process; the legs alternate.  Latent in, latent out.

    python tools/bench_redux.py [--size 1024] [--steps 28] [--iters 1] [--rounds 2] [--warmup 1] [--in-flight 2] [--prior-iters 5] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--iters", type=int, default=1, help="loops per leg and round")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--in-flight", type=int, default=2)
    ap.add_argument("--prior-iters", type=int, default=5, help="timed images through the prior")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redux_bench.json"), help="where the JSON line is written")
    a = ap.parse_args()
    from thinkdiff import _hip
    from thinkdiff.models.flux_prompt import FlowMatchEulerSchedule
    from thinkdiff.models.flux_redux import FluxPriorReduxPipelineRewritePrompt, ReduxDefaultImageProcessor, ReduxImageEncoder
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig, effective_scalar
    from thinkdiff.models.vision_towers import HipSiglipVisionModel

    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)

    # ---- the prior, per image -----------------------------------------------------------------------------------------------------
    tower, embedder = HipSiglipVisionModel.from_random(seed=11), ReduxImageEncoder.from_random(seed=12)
    prior = FluxPriorReduxPipelineRewritePrompt(tower, ReduxDefaultImageProcessor(), embedder)
    pix = torch.randn(1, 3, 384, 384, generator=g).cuda()
    calls = [0]
    check = _hip.check

    def counting_check(status):
        calls[0] += 1
        return check(status)

    parts = {"tower": lambda st: st.update(hs=tower(pix).last_hidden_state),
             "mlp": lambda st: st.update(emb=embedder(st["hs"]).image_embeds.contiguous()),
             "compose": lambda st: st.update(pe=_hip.redux_compose(None, st["emb"], [1.0], T=512),
                                             pool=_hip.redux_compose(None, None, [1.0], T=1, D=768, device=pix.device))}
    state, prior_ms, prior_calls = {}, {}, {}
    for name, fn in parts.items():
        _hip.check = counting_check
        calls[0] = 0
        fn(state)                                           # warm-up, and the call count
        prior_calls[name] = calls[0]
        _hip.check = check
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.prior_iters):
            fn(state)
        e1.record()
        torch.cuda.synchronize()
        prior_ms[name] = e0.elapsed_time(e1) / a.prior_iters
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.prior_iters):
        out = prior(pix)
    torch.cuda.synchronize()
    prior_wall_ms = (time.perf_counter() - t0) / a.prior_iters * 1e3
    assert out["prompt_embeds"].shape == (1, 512 + 729, 4096) and bool(torch.isfinite(out["prompt_embeds"].float()).all())
    redux_stream = out["prompt_embeds"][0].clone()
    del tower, embedder, prior, state, parts
    torch.cuda.empty_cache()

    # ---- the denoise loop at both stream lengths -------------------------------------------------------------------------------------
    n_side = a.size // 16
    S, G, n = n_side * n_side, max(1, a.in_flight), a.steps
    T_long = redux_stream.shape[0]
    cfg = FluxTransformerConfig()
    J = cfg.joint_attention_dim
    tr = FluxTransformer2DModel(cfg, max_img_tokens=S, max_txt_tokens=T_long, max_steps=max(32, n)).init_random(1234)      # max_txt_tokens >= T + 729
    ctxs = [tr] + [tr.fork() for _ in range(G - 1)]
    streams = [torch.cuda.Stream() for _ in range(G)]
    pe = {"t512": torch.randn(512, J, generator=g).bfloat16().cuda(), f"t{T_long}": torch.randn(T_long, J, generator=g).bfloat16().cuda()}
    pooled = torch.randn(768, generator=g).bfloat16().cuda()
    lat0 = torch.randn(S, 64, generator=g).bfloat16().cuda()
    ids = torch.zeros(n_side, n_side, 3)
    ids[..., 1] += torch.arange(n_side)[:, None]
    ids[..., 2] += torch.arange(n_side)[None, :]
    ids = ids.reshape(S, 3).cuda()
    sig = FlowMatchEulerSchedule().sigmas(n, S)
    t_eff = [effective_scalar(float(s) * 1000.0, torch.bfloat16) for s in sig[:-1]]
    g_eff = float((torch.tensor([3.5]).bfloat16() * 1000).float())

    def loop(leg):
        xs = []
        for k in range(G):
            ctxs[k].set_condition(pe[leg], pooled, ids)
            ctxs[k].set_timesteps(t_eff, g_eff)
            xs.append(lat0.clone())
        torch.cuda.synchronize()
        if G == 1:
            ctxs[0].denoise(xs[0], sig)
        else:
            FluxTransformer2DModel.denoise_multi(ctxs, xs, sig, streams)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xs[0].float()).all())

    legs = list(pe)

    def rate(leg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            loop(leg)
        return G * a.iters / (time.perf_counter() - t0)

    for _ in range(a.warmup):
        for leg in legs:
            loop(leg)
    rounds = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg in legs:
            rounds[leg].append(rate(leg))
    mean = {k: sum(v) / len(v) for k, v in rounds.items()}
    short, long_ = legs
    res = {"metric": "redux", "size": a.size, "steps": n, "in_flight": G, "tower": "siglip-so400m-patch14-384 shape, 27 layers, 729 tokens",
           "prior_ms": {k: round(v, 3) for k, v in prior_ms.items()}, "prior_ms_total": round(sum(prior_ms.values()), 3),
           "prior_wall_ms_per_image": round(prior_wall_ms, 3), "prior_c_abi_calls": prior_calls,
           f"{short}_images_per_s": round(mean[short], 4), f"{long_}_images_per_s": round(mean[long_], 4),
           "time_ratio_long_vs_short": round(mean[short] / mean[long_], 4),
           "row_arithmetic": {"linears": round((S + T_long) / (S + 512), 4), "joint_attention": round(((S + T_long) / (S + 512)) ** 2, 4)},
           "rounds": {k: [round(x, 4) for x in v] for k, v in rounds.items()}}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
