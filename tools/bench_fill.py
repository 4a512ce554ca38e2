"""FLUX.1 Fill at 1024 x 1024 on a full-size synthetic 384 / 64-channel transformer and VAE against text-to-image on a full-size
64 / 64 transformer in the same process: one JSON line with
  * fill_images_per_s        -- FluxFillPipelineRewritePrompt(image=PIL, mask_image=PIL) end to end, uint8 out, the full schedule
  * t2i_images_per_s         -- FluxPipelineRewritePrompt at the same steps / size / images in flight, alternated with Fill (A B A B)
  * fill_vs_t2i              -- the ratio of the two rates (equal forward count: both run every step of the schedule)
  * the per-image stages Fill adds: host mask conversion, the masked encode against the plain one, the condition kernel, the copy
    of the condition into the engine context (ms / us each)
The x_embedder gather (td_copy_cols_kernel, once per forward) has no entry point of its own: read it off a kernel trace of this tool
(`rocprofv3 --kernel-trace --stats -- python tools/bench_fill.py --iters 1 --rounds 1`).

    python tools/bench_fill.py [--size 1024] [--steps 28] [--iters 2] [--rounds 2] [--warmup 1] [--in-flight 2] [--launches 200]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def device_us(fn, launches):
    """Device time per launch (HIP events around `launches` back-to-back launches, after as many warm ones)."""
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def host_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--iters", type=int, default=2, help="calls per leg")
    ap.add_argument("--rounds", type=int, default=2, help="A B rounds (fill, text-to-image)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--in-flight", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    from PIL import Image
    from thinkdiff.models.flux_fill import FluxFillPipelineRewritePrompt
    from thinkdiff.models.flux_inpaint import preprocess_mask
    from thinkdiff.models.flux_prompt import FluxPipelineRewritePrompt
    from thinkdiff.models.flux_transformer import _OPS, FluxTransformer2DModel, FluxTransformerConfig
    from thinkdiff.models.flux_vae import AutoencoderKLEncoder

    torch.cuda.set_device(0)
    S = a.size
    n_tok = (S // 16) ** 2
    t2i = FluxPipelineRewritePrompt.from_random(seed=1234, max_img_tokens=n_tok, max_txt_tokens=512, max_steps=max(32, a.steps))
    t2i.images_in_flight = max(1, a.in_flight)
    # fork the contexts and make the streams once, before the second pipeline is built, and run both pipelines on the SAME streams: streams
    # made later than others share the process's hardware queues differently, which alone moved a rate by ~4 % in one process
    t2i._contexts(t2i.images_in_flight)
    enc = AutoencoderKLEncoder(max_image_size=(S, S)).init_random(seed=1236)
    tr_fill = FluxTransformer2DModel(FluxTransformerConfig(in_channels=384, out_channels=64), max_img_tokens=n_tok, max_txt_tokens=512,
                                     max_steps=max(32, a.steps)).init_random(1235)
    fill = FluxFillPipelineRewritePrompt(transformer=tr_fill, vae=t2i.vae, vae_encoder=enc)
    fill.images_in_flight = t2i.images_in_flight
    fill._ctx_pool, fill._streams = [tr_fill], t2i._streams
    fill._contexts(fill.images_in_flight)
    assert fill._streams is t2i._streams and len(fill._ctx_pool) == len(t2i._ctx_pool)
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (S, S, 3), generator=g, dtype=torch.uint8)
    u8 = torch.nn.functional.avg_pool2d(u8.permute(2, 0, 1)[None].float(), 9, 1, 4)[0].permute(1, 2, 0).round().to(torch.uint8)
    img = Image.fromarray(u8.numpy())
    mk = np.zeros((S, S), np.uint8)
    mk[S // 4: 3 * S // 4, S // 4: 3 * S // 4] = 255          # fill the centre quarter
    mask = Image.fromarray(mk, "L")
    pe = torch.randn(1, 193, 4096, generator=g).bfloat16().cuda()
    pooled = torch.randn(1, 768, generator=g).bfloat16().cuda()
    B = max(1, a.in_flight)                                  # one prompt x B images: B in flight
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pooled, height=S, width=S, num_inference_steps=a.steps, guidance_scale=3.5,
              num_images_per_prompt=B, output_type="np")

    def call(p, **extra):
        out = p(generator=torch.Generator(device="cuda").manual_seed(1), **kw, **extra).images
        assert out.shape == (B, S, S, 3)

    legs = {"fill": lambda: call(fill, image=img, mask_image=mask), "t2i": lambda: call(t2i)}

    def rate(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            legs[name]()
        torch.cuda.synchronize()
        return B * a.iters / (time.perf_counter() - t0)

    for _ in range(a.warmup):
        legs["fill"]()
        legs["t2i"]()
    r_fill, r_t2i = [], []
    for _ in range(a.rounds):
        r_fill.append(rate("fill"))
        r_t2i.append(rate("t2i"))

    # the per-image stages Fill adds to text-to-image
    h = S // 8
    mask_host = host_ms(lambda: preprocess_mask(mask, S, S), 5)
    m_dev = preprocess_mask(mask, S, S)[0].cuda()
    u8_dev = u8.cuda()
    enc_plain = host_ms(lambda: enc.encode_moments(u8_dev), 3)
    enc_masked = host_ms(lambda: enc.encode_moments(u8_dev, mask=m_dev), 3)
    mom = enc.encode_moments(u8_dev, mask=m_dev)
    eps = torch.randn((16, h, h), device="cuda", dtype=torch.bfloat16)
    cond_us = device_us(lambda: _OPS.flux_fill_condition(mom, eps, m_dev, 0.3611, 0.1159, S, S), a.launches)
    cond = _OPS.flux_fill_condition(mom, eps, m_dev, 0.3611, 0.1159, S, S)
    set_us = device_us(lambda: _OPS.flux_set_channel_condition(int(tr_fill._h.value), cond), a.launches)

    f, t = sum(r_fill) / len(r_fill), sum(r_t2i) / len(r_t2i)
    res = {"metric": "fill", "size": S, "steps": a.steps, "images_per_call": B, "in_flight": fill.images_in_flight,
           "fill_images_per_s": round(f, 4), "t2i_images_per_s": round(t, 4), "fill_vs_t2i": round(f / t, 4),
           "fill_rounds": [round(r, 4) for r in r_fill], "t2i_rounds": [round(r, 4) for r in r_t2i],
           "mask_host_ms": round(mask_host, 3), "encode_ms": round(enc_plain, 3), "masked_encode_ms": round(enc_masked, 3),
           "fill_condition_kernel_us": round(cond_us, 2), "fill_condition_bytes": n_tok * 320 * 2 + S * S + h * h * 32 * 2 + 16 * h * h * 2,
           "set_channel_condition_us": round(set_us, 2)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
