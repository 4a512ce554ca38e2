"""FLUX image-to-image at 1024 x 1024 on the full-size synthetic FLUX.1 transformer and VAE: one JSON line with
  * encoder_ms       -- td_vae_encode (image-in kernel + Encoder) of one uint8 image, device time per call (HIP events)
  * encoder_tflops   -- its executed FLOPs (counted from the layer shapes below, conv_in's zero-padded input channels included) / time
  * decode_ms        -- td_vae_decode of one 128 x 128 latent (the text-to-image tail), same process and weights scheme
  * img2img_images_per_s -- FluxImg2ImgPipelineRewritePrompt(image=PIL, strength, num_inference_steps) end to end, uint8 out

    python tools/bench_img2img.py [--size 1024] [--steps 28] [--strength 0.6] [--iters 3] [--warmup 1] [--in-flight 2]
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


def encoder_flops(H, W, boc=(128, 256, 512, 512), layers=2, latent=16, cin_pad=64):
    """Multiply-adds x 2 of every GEMM the encoder launches at an H x W image."""
    f = 0
    conv = lambda P, cin, cout: 2 * P * cout * 9 * cin
    P = H * W
    f += conv(P, cin_pad, boc[0])
    prev = boc[0]
    for b, co in enumerate(boc):
        for r in range(layers):
            cin = prev if r == 0 else co
            f += conv(P, cin, co) + conv(P, co, co) + (2 * P * cin * co if cin != co else 0)
        if b != len(boc) - 1:
            P //= 4
            f += conv(P, co, co)
        prev = co
    c = boc[-1]
    f += 2 * (conv(P, c, c) * 2)                       # two mid-block resnets
    f += 4 * 2 * P * c * c + 2 * 2 * P * P * c        # q, k, v, out projections; scores and P.V
    f += conv(P, c, 2 * latent)
    return f


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--strength", type=float, default=0.6)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--in-flight", type=int, default=2)
    a = ap.parse_args()
    from PIL import Image
    from thinkdiff.models.flux_img2img import FluxImg2ImgPipelineRewritePrompt, get_timesteps
    from thinkdiff.models.flux_prompt import FluxPipelineRewritePrompt
    from thinkdiff.models.flux_vae import AutoencoderKLEncoder

    torch.cuda.set_device(0)
    S = a.size
    pipe = FluxPipelineRewritePrompt.from_random(seed=1234, max_img_tokens=4096, max_txt_tokens=512, max_steps=32)
    pipe.images_in_flight = max(1, a.in_flight)
    enc = AutoencoderKLEncoder(max_image_size=(S, S)).init_random(seed=1236)
    i2i = FluxImg2ImgPipelineRewritePrompt.from_pipe(pipe, enc)
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (S, S, 3), generator=g, dtype=torch.uint8)
    u8 = torch.nn.functional.avg_pool2d(u8.permute(2, 0, 1)[None].float(), 9, 1, 4)[0].permute(1, 2, 0).round().to(torch.uint8)
    img = Image.fromarray(u8.numpy())
    u8_dev = u8.cuda()
    pe = torch.randn(1, 193, 4096, generator=g).bfloat16().cuda()
    pooled = torch.randn(1, 768, generator=g).bfloat16().cuda()

    enc_ms = timed(lambda: enc.encode_moments(u8_dev), max(5, a.iters), a.warmup + 1)
    h = S // 8
    lat = torch.randn((h // 2) * (h // 2), 64, generator=g).bfloat16().cuda()
    dec_ms = timed(lambda: pipe.vae.decode_packed(lat, h, h, output_type="np"), max(5, a.iters), a.warmup + 1)

    def call():
        return i2i(image=img, strength=a.strength, prompt_embeds=pe, pooled_prompt_embeds=pooled, height=S, width=S,
                   num_inference_steps=a.steps, guidance_scale=3.5, generator=torch.Generator(device="cuda").manual_seed(1), output_type="np").images
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = call()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    assert out.shape == (1, S, S, 3)
    fl = encoder_flops(S, S)
    res = {"metric": "img2img", "size": S, "steps": a.steps, "strength": a.strength,
           "denoise_steps": a.steps - get_timesteps(a.steps, a.strength), "in_flight": pipe.images_in_flight,
           "encoder_ms": round(enc_ms, 3), "encoder_tflop": round(fl / 1e12, 3), "encoder_tflops": round(fl / (enc_ms * 1e-3) / 1e12, 1),
           "decode_ms": round(dec_ms, 3), "img2img_images_per_s": round(a.iters / el, 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
