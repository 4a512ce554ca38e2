"""FLUX IP-Adapter at 1024 x 1024 on a full-size synthetic FLUX.1-dev transformer, random weights, against text-to-image in the same process:
one JSON line with
  * plain_images_per_s       -- the plain denoise loop (condition, schedule, td_flux_denoise_multi), `--in-flight` images at once, adapters loaded
                                but no image prompt set (the plain forward's launches)
  * ip4_images_per_s         -- the same loop with the image prompt of a 4-token adapter (E = 768) on every context, scale 0.7
  * ip128_images_per_s       -- ... of a 128-token adapter (E = 1152)
  * ip_attention_us          -- td_ip_attention_bf16 alone at rows = S_img, H = 24 on the image rows of a [T + S_img, 3 D] buffer, 4 and 128 keys
and the ratios to the plain rate beside the traffic estimate (per double block: q read, the [S_img, D] buffer written, then read with h and h
written back = 5 S_img D 2 bytes).  The yardstick is the plain rate of THIS process; the legs alternate (A B C rounds).  Latent in, latent out.

    python tools/bench_ip_adapter.py [--size 1024] [--steps 28] [--iters 1] [--rounds 2] [--warmup 1] [--in-flight 2] [--launches 200] [--out FILE]
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


def synthetic_adapter(num_tokens, E, L, J, D, seed):
    """A full-shape adapter drawn on the device (the stds of the tests' fixture)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda std, *shape: (std * torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32)).bfloat16()
    proj = {"proj.weight": rn(0.05, num_tokens * J, E), "proj.bias": rn(0.02, num_tokens * J), "norm.weight": 1.0 + rn(0.1, J), "norm.bias": rn(0.05, J)}
    blocks = {}
    for i in range(L):
        blocks[f"{i}.to_k_ip.weight"], blocks[f"{i}.to_k_ip.bias"] = rn(0.02, D, J), rn(0.02, D)
        blocks[f"{i}.to_v_ip.weight"], blocks[f"{i}.to_v_ip.bias"] = rn(0.004, D, J), rn(0.004, D)
    return {"image_proj": proj, "ip_adapter": blocks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--iters", type=int, default=1, help="loops per leg and round")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--in-flight", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200, help="timed launches of td_ip_attention_bf16 per key count")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from thinkdiff.models.flux_prompt import FlowMatchEulerSchedule
    from thinkdiff.models.flux_transformer import _OPS, FluxTransformer2DModel, FluxTransformerConfig, effective_scalar

    torch.cuda.set_device(0)
    n_side = a.size // 16
    S, T, G, n = n_side * n_side, 193, max(1, a.in_flight), a.steps
    cfg = FluxTransformerConfig()
    L, J, D, H = cfg.num_layers, cfg.joint_attention_dim, cfg.inner_dim, cfg.num_attention_heads
    tr = FluxTransformer2DModel(cfg, max_img_tokens=S, max_txt_tokens=512, max_steps=max(32, n)).init_random(1234)
    adapters = {"ip4": (4, 768), "ip128": (128, 1152)}
    index = {}
    for name, (nt, E) in adapters.items():
        index[name] = tr.load_ip_adapter(synthetic_adapter(nt, E, L, J, D, 77 + nt))
    tr.set_ip_adapter_scale(0.7)
    ctxs = [tr] + [tr.fork() for _ in range(G - 1)]
    streams = [torch.cuda.Stream() for _ in range(G)]
    g = torch.Generator().manual_seed(0)
    pe = torch.randn(T, J, generator=g).bfloat16().cuda()
    pooled = torch.randn(768, generator=g).bfloat16().cuda()
    lat0 = torch.randn(S, 64, generator=g).bfloat16().cuda()
    embeds = {name: torch.randn(1, E, generator=g).bfloat16().cuda() for name, (_, E) in adapters.items()}
    ids = torch.zeros(n_side, n_side, 3)
    ids[..., 1] += torch.arange(n_side)[:, None]
    ids[..., 2] += torch.arange(n_side)[None, :]
    ids = ids.reshape(S, 3).cuda()
    sig = FlowMatchEulerSchedule().sigmas(n, S)
    t_eff = [effective_scalar(float(s) * 1000.0, torch.bfloat16) for s in sig[:-1]]
    g_eff = float((torch.tensor([3.5]).bfloat16() * 1000).float())

    def loop(leg):
        """One group of G images: condition, image prompt (or none) and schedule on every context, then the loop."""
        xs = []
        for k in range(G):
            ctxs[k].set_condition(pe, pooled, ids)
            ctxs[k].set_ip_image_embeds(None)
            if leg != "plain":      # (the other adapter stays without an image prompt on this context: it launches nothing)
                _OPS.flux_set_ip_image_embeds(int(ctxs[k]._h.value), tr.ip_adapters()[index[leg]]["slot"], embeds[leg])
            ctxs[k].set_timesteps(t_eff, g_eff)
            xs.append(lat0.clone())
        torch.cuda.synchronize()
        if G == 1:
            ctxs[0].denoise(xs[0], sig)
        else:
            FluxTransformer2DModel.denoise_multi(ctxs, xs, sig, streams)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xs[0].float()).all())

    legs = ["plain", "ip4", "ip128"]

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

    # the kernel alone: the image rows of a joint [T + S, 3 D] projection buffer, K / V [n_keys, D], output [S, D]
    qkv = torch.randn(T + S, 3 * D, generator=g).bfloat16().cuda()
    out = torch.empty(S, D, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(128, dtype=torch.bfloat16, device="cuda")
    kernel_us = {}
    for n_keys in (4, 128):
        k = torch.randn(n_keys, D, generator=g).bfloat16().cuda()
        v = torch.randn(n_keys, D, generator=g).bfloat16().cuda()
        run = lambda: _OPS.ip_attention_(out, qkv[T:, :D], k, v, H, w, 1e-6, 0.7, False)
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            run()
        e1.record()
        torch.cuda.synchronize()
        kernel_us[n_keys] = e0.elapsed_time(e1) / a.launches * 1e3

    mean = {k: sum(v) / len(v) for k, v in rounds.items()}
    traffic_block = 5 * S * D * 2      # q read, ip written; ip read, h read, h written
    res = {"metric": "ip_adapter", "size": a.size, "steps": n, "in_flight": G, "adapters": {k: {"num_tokens": v[0], "embed_dim": v[1]} for k, v in adapters.items()},
           "plain_images_per_s": round(mean["plain"], 4), "ip4_images_per_s": round(mean["ip4"], 4), "ip128_images_per_s": round(mean["ip128"], 4),
           "ip4_vs_plain": round(mean["ip4"] / mean["plain"], 4), "ip128_vs_plain": round(mean["ip128"] / mean["plain"], 4),
           "rounds": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
           "traffic_bytes_per_double_block": traffic_block, "traffic_gb_per_step": round(L * traffic_block / 1e9, 3),
           "ip_attention_us": {str(k): round(v, 2) for k, v in kernel_us.items()},
           "ip_attention_gb_per_s": {str(k): round(2 * S * D * 2 / (v * 1e-6) / 1e9, 1) for k, v in kernel_us.items()},
           "ip_attention_rows": S, "ip_attention_heads": H}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
