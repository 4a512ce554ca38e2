"""FLUX ControlNet at 1024 x 1024 on a full-size synthetic FLUX.1-dev transformer and a ControlNet of the InstantX Union shape (5 double
+ 10 single blocks, num_mode 10, no guidance embedder), random weights, against text-to-image in the same process: one JSON line with
  * t2i_images_per_s            -- the plain denoise loop (condition, schedule, td_flux_denoise_multi), `--in-flight` images at once
  * cn_scale1_images_per_s      -- the same loop with one ControlNet fork attached per context, conditioning scale 1 at every step
  * cn_end_half_images_per_s    -- control_guidance_end = 0.5: the second half of the schedule runs the plain step
  * cn_scale0_images_per_s      -- attached, scale 0 at every step: the plain forward's launches
  * inject_ms_per_step          -- flux_residual_inject_ on [S_img, D] rows of a [T + S_img, D] buffer, 57 launches (one per main block), summed
and the ratios to text-to-image beside the block-count model 57 / (57 + n_d + n_s + (n_d + n_s) / 12).  The legs alternate (A B C D
rounds).  Latent in, latent out: the control image's VAE pass is img2img's and is not timed here.

    python tools/bench_controlnet.py [--size 1024] [--steps 28] [--iters 1] [--rounds 2] [--warmup 1] [--in-flight 2] [--launches 50] [--out FILE]
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
    from thinkdiff.models.flux_controlnet import FluxControlNetConfig, FluxControlNetModel, controlnet_keep
    from thinkdiff.models.flux_prompt import FlowMatchEulerSchedule
    from thinkdiff.models.flux_transformer import _OPS, FluxTransformer2DModel, FluxTransformerConfig, effective_scalar

    torch.cuda.set_device(0)
    n_side = a.size // 16
    S, T, G, n = n_side * n_side, 193, max(1, a.in_flight), a.steps
    caps = dict(max_img_tokens=S, max_txt_tokens=512, max_steps=max(32, n))
    tr = FluxTransformer2DModel(FluxTransformerConfig(), **caps).init_random(1234)
    cfg_cn = FluxControlNetConfig(num_layers=5, num_single_layers=10, num_mode=10, guidance_embeds=False)
    cn = FluxControlNetModel(cfg_cn, **caps).init_random(1235)
    ctxs, cns = [tr] + [tr.fork() for _ in range(G - 1)], [cn] + [cn.fork() for _ in range(G - 1)]
    streams = [torch.cuda.Stream() for _ in range(G)]
    g = torch.Generator().manual_seed(0)
    pe = torch.randn(T, 4096, generator=g).bfloat16().cuda()
    pooled = torch.randn(768, generator=g).bfloat16().cuda()
    lat0 = torch.randn(S, 64, generator=g).bfloat16().cuda()
    cond = torch.randn(S, 64, generator=g).bfloat16().cuda()
    ids = torch.zeros(n_side, n_side, 3)
    ids[..., 1] += torch.arange(n_side)[:, None]
    ids[..., 2] += torch.arange(n_side)[None, :]
    ids = ids.reshape(S, 3).cuda()
    sig = FlowMatchEulerSchedule().sigmas(n, S)
    t_eff = [effective_scalar(float(s) * 1000.0, torch.bfloat16) for s in sig[:-1]]
    g_eff = float((torch.tensor([3.5]).bfloat16() * 1000).float())

    def loop(scales):
        """One group of G images: condition + schedule on every context (and on its ControlNet fork when scales is given), then the loop."""
        xs = []
        for k in range(G):
            ctxs[k].set_condition(pe, pooled, ids)
            ctxs[k].set_timesteps(t_eff, g_eff)
            if scales is not None:
                cns[k].set_condition(pe, pooled, ids, control_mode=0)
                cns[k].set_control_condition(cond)
                cns[k].set_timesteps(t_eff, 0.0)
                ctxs[k].attach_controlnet(cns[k])
                ctxs[k].set_controlnet_scales(scales)
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
                ctxs[k].attach_controlnet(None)
        assert bool(torch.isfinite(xs[0].float()).all())

    legs = {"t2i": None, "cn_scale1": [1.0] * n, "cn_end_half": controlnet_keep(n, 0.0, 0.5), "cn_scale0": [0.0] * n}

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

    # the injection alone: image rows of a joint [T + S, D] buffer, a [S, D] sample, one launch per block of the main model
    D, blocks = 3072, 19 + 38
    h = torch.randn(T + S, D, generator=g).bfloat16().cuda()
    r = torch.randn(S, D, generator=g).bfloat16().cuda()

    def inject_all():
        for _ in range(blocks):
            _OPS.flux_residual_inject_(h[T:], r, 0.7)

    inject_all()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches):
        inject_all()
    e1.record()
    torch.cuda.synchronize()
    inject_ms = e0.elapsed_time(e1) / a.launches

    mean = {k: sum(v) / len(v) for k, v in rounds.items()}
    n_d, n_s = cfg_cn.num_layers, cfg_cn.num_single_layers
    res = {"metric": "controlnet", "size": a.size, "steps": n, "in_flight": G, "controlnet": {"num_layers": n_d, "num_single_layers": n_s, "num_mode": 10,
                                                                                                 "guidance_embeds": False},
           "t2i_images_per_s": round(mean["t2i"], 4), "cn_scale1_images_per_s": round(mean["cn_scale1"], 4),
           "cn_end_half_images_per_s": round(mean["cn_end_half"], 4), "cn_scale0_images_per_s": round(mean["cn_scale0"], 4),
           "cn_scale1_vs_t2i": round(mean["cn_scale1"] / mean["t2i"], 4), "cn_end_half_vs_t2i": round(mean["cn_end_half"] / mean["t2i"], 4),
           "cn_scale0_vs_t2i": round(mean["cn_scale0"] / mean["t2i"], 4),
           "model_scale1_vs_t2i": round(blocks / (blocks + n_d + n_s + (n_d + n_s) / 12.0), 4),
           "rounds": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
           "inject_ms_per_step": round(inject_ms, 4), "inject_launches_per_step": blocks,
           "inject_bytes_per_launch": 3 * S * D * 2, "inject_gb_per_s": round(blocks * 3 * S * D * 2 / (inject_ms * 1e-3) / 1e9, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
