"""Two FLUX ControlNets at 1024 x 1024 on a full-size synthetic FLUX.1-dev transformer, against one ControlNet and against text-to-image
in the same process.  The ControlNet has the InstantX Union shape (5 double + 10 single blocks, num_mode 10, no guidance embedder), random
weights; the two-net leg lists it TWICE -- the form the Union checkpoints are published for: one union net under two modes with two control
images -- so every main context is paired with two forks of it.  One JSON line with
  * t2i_images_per_s           -- the plain denoise loop (condition, schedule, td_flux_denoise_multi), `--in-flight` images at once
  * cn1_images_per_s           -- one ControlNet fork attached per context, conditioning scale 1 at every step
  * cn2_images_per_s           -- two forks attached per context (modes 0 and 1, two control images), scales 1 and 0.6 at every step
  * cn2_windows_images_per_s   -- the same with per-net guidance windows: net 0 over [0, 0.5], net 1 over [0.25, 1]
  * inject1_ms_per_step / inject2_ms_per_step / inject2_as_two_ms_per_step -- the injection alone on [S_img, D] rows of a [T + S_img, D]
    buffer, 57 launches (one per main block): flux_residual_inject_ with one sample, flux_residual_inject_multi_ with two, and two
    flux_residual_inject_ launches per block (what the fused sum replaces -- other values, and one more pass over the rows)
and the ratios to text-to-image beside the block-count model 57 / (57 + K (n_d + n_s + (n_d + n_s) / 12)).  The legs alternate (A B C D
rounds).  Latent in, latent out: the control images' VAE passes are img2img's and are not timed here.

    python tools/bench_multi_controlnet.py [--size 1024] [--steps 28] [--iters 1] [--rounds 2] [--warmup 1] [--in-flight 2] [--launches 50] [--out FILE]
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
    ap.add_argument("--launches", type=int, default=50, help="timed repetitions of the 57 inject launches")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from thinkdiff.models.flux_controlnet import FluxControlNetConfig, FluxControlNetModel, controlnet_scale_tables
    from thinkdiff.models.flux_prompt import FlowMatchEulerSchedule
    from thinkdiff.models.flux_transformer import _OPS, FluxTransformer2DModel, FluxTransformerConfig, effective_scalar

    torch.cuda.set_device(0)
    n_side = a.size // 16
    S, T, G, n = n_side * n_side, 193, max(1, a.in_flight), a.steps
    caps = dict(max_img_tokens=S, max_txt_tokens=512, max_steps=max(32, n))
    tr = FluxTransformer2DModel(FluxTransformerConfig(), **caps).init_random(1234)
    cfg_cn = FluxControlNetConfig(num_layers=5, num_single_layers=10, num_mode=10, guidance_embeds=False)
    cn = FluxControlNetModel(cfg_cn, **caps).init_random(1235)
    ctxs = [tr] + [tr.fork() for _ in range(G - 1)]
    cns = [[cn if k == 0 else cn.fork(), cn.fork()] for k in range(G)]      # per main context: two contexts of the one model
    streams = [torch.cuda.Stream() for _ in range(G)]
    g = torch.Generator().manual_seed(0)
    pe = torch.randn(T, 4096, generator=g).bfloat16().cuda()
    pooled = torch.randn(768, generator=g).bfloat16().cuda()
    lat0 = torch.randn(S, 64, generator=g).bfloat16().cuda()
    conds = [torch.randn(S, 64, generator=g).bfloat16().cuda() for _ in range(2)]
    ids = torch.zeros(n_side, n_side, 3)
    ids[..., 1] += torch.arange(n_side)[:, None]
    ids[..., 2] += torch.arange(n_side)[None, :]
    ids = ids.reshape(S, 3).cuda()
    sig = FlowMatchEulerSchedule().sigmas(n, S)
    t_eff = [effective_scalar(float(s) * 1000.0, torch.bfloat16) for s in sig[:-1]]
    g_eff = float((torch.tensor([3.5]).bfloat16() * 1000).float())

    def loop(tables):
        """One group of G images: condition + schedule on every context (and on len(tables) of its ControlNet forks), then the loop."""
        xs = []
        for k in range(G):
            ctxs[k].set_condition(pe, pooled, ids)
            ctxs[k].set_timesteps(t_eff, g_eff)
            if tables:
                for j in range(len(tables)):
                    cns[k][j].set_condition(pe, pooled, ids, control_mode=j)
                    cns[k][j].set_control_condition(conds[j])
                    cns[k][j].set_timesteps(t_eff, 0.0)
                ctxs[k].attach_controlnets(cns[k][:len(tables)])
                for j, tab in enumerate(tables):
                    ctxs[k].set_controlnet_scales(tab, net=j)
            xs.append(lat0.clone())
        torch.cuda.synchronize()
        try:
            if G == 1:
                ctxs[0].denoise(xs[0], sig)
            else:
                FluxTransformer2DModel.denoise_multi(ctxs, xs, sig, streams)
            torch.cuda.synchronize()
        finally:
            for k in range(G):
                ctxs[k].attach_controlnets([])
        assert bool(torch.isfinite(xs[0].float()).all())

    legs = {"t2i": None, "cn1": controlnet_scale_tables(n, 1), "cn2": controlnet_scale_tables(n, 2, [1.0, 0.6]),
            "cn2_windows": controlnet_scale_tables(n, 2, [1.0, 0.6], [0.0, 0.25], [0.5, 1.0])}

    def rate(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            loop(legs[name])
        return G * a.iters / (time.perf_counter() - t0)

    for _ in range(a.warmup):
        for name in legs:
            loop(legs[name])
    rounds = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name in legs:
            rounds[name].append(rate(name))

    # the injection alone: image rows of a joint [T + S, D] buffer, [S, D] samples, one launch (or two) per block of the main model
    D, blocks = 3072, 19 + 38
    h = torch.randn(T + S, D, generator=g).bfloat16().cuda()
    r = [torch.randn(S, D, generator=g).bfloat16().cuda() for _ in range(2)]

    def timed(fn):
        for _ in range(blocks):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches * blocks):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches

    def two_singles():
        _OPS.flux_residual_inject_(h[T:], r[0], 0.7)
        _OPS.flux_residual_inject_(h[T:], r[1], 0.45)

    inj1 = timed(lambda: _OPS.flux_residual_inject_(h[T:], r[0], 0.7))
    inj2 = timed(lambda: _OPS.flux_residual_inject_multi_(h[T:], r, [0.7, 0.45]))
    inj11 = timed(two_singles)

    mean = {k: sum(v) / len(v) for k, v in rounds.items()}
    n_d, n_s = cfg_cn.num_layers, cfg_cn.num_single_layers
    side = n_d + n_s + (n_d + n_s) / 12.0
    active = {k: (sum(1 for tab in v for s in tab if s != 0.0) / n if v else 0.0) for k, v in legs.items()}      # net evaluations per step
    res = {"metric": "multi_controlnet", "size": a.size, "steps": n, "in_flight": G,
           "controlnet": {"num_layers": n_d, "num_single_layers": n_s, "num_mode": 10, "guidance_embeds": False, "listed_twice": True},
           "t2i_images_per_s": round(mean["t2i"], 4), "cn1_images_per_s": round(mean["cn1"], 4), "cn2_images_per_s": round(mean["cn2"], 4),
           "cn2_windows_images_per_s": round(mean["cn2_windows"], 4),
           "cn1_vs_t2i": round(mean["cn1"] / mean["t2i"], 4), "cn2_vs_t2i": round(mean["cn2"] / mean["t2i"], 4),
           "cn2_windows_vs_t2i": round(mean["cn2_windows"] / mean["t2i"], 4),
           "model_cn1_vs_t2i": round(blocks / (blocks + side), 4), "model_cn2_vs_t2i": round(blocks / (blocks + 2 * side), 4),
           "model_cn2_windows_vs_t2i": round(blocks / (blocks + active["cn2_windows"] * side), 4),
           "net_evaluations_per_step": {k: round(v, 4) for k, v in active.items()},
           "rounds": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
           "inject1_ms_per_step": round(inj1, 4), "inject2_ms_per_step": round(inj2, 4), "inject2_as_two_ms_per_step": round(inj11, 4),
           "inject_launches_per_step": blocks, "inject1_bytes_per_launch": 3 * S * D * 2, "inject2_bytes_per_launch": 4 * S * D * 2,
           "inject1_gb_per_s": round(blocks * 3 * S * D * 2 / (inj1 * 1e-3) / 1e9, 1), "inject2_gb_per_s": round(blocks * 4 * S * D * 2 / (inj2 * 1e-3) / 1e9, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
