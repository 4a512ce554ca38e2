"""LoRA adapter changes on a full-size synthetic FLUX.1-dev transformer (init_random), adapters on every block Linear (attn.*, ff*, proj_mlp,
the single blocks' proj_out: 418 parameters, 11.3 G elements), in one process: one JSON object with, per case (one adapter at rank 16 / 64 /
128, two adapters of rank 64):
  * set_adapters_ms           -- td_flux_lora_set_adapters end to end, device events around the call, warmed, `--reps` repetitions: median, min, max
                                 (a CALL time: 418 merge launches back to back, not a kernel's share of peak)
  * copy_ms                   -- yardstick 1, same process: hipMemcpyDtoDAsync of the same parameter bytes, parameter by parameter (the same 2 B in
                                 + 2 B out per element and the same launch count, no arithmetic); ratio_to_copy = set_adapters / copy, the bar is 1.25
  * operand_share_3072        -- (N + K) R 2 / (N K 4) on a 3072 x 3072 Linear: what the adapter operands add to the weight traffic, from shapes
  * torch_ms                  -- yardstick 2: what a user of the parent commit would write with torch on the device had they the base weights:
                                 per parameter (W.float() + s (B.float() @ A.float())).bfloat16() and td_flux_load_param; ratio only, no bar
  * int8: set_adapters_ms with the re-quantisation it then includes, and requant_ms (td_flux_set_precision alone) beside it
  * bytes_held (td_flux_lora_info), set_adapters as a share of one 28-step 1024^2 image, images/s with the adapter merged and without.
For the merge kernel alone read a kernel trace of this tool: `rocprofv3 --kernel-trace --stats -- python tools/bench_lora.py --reps 5 --skip-image`.

    python tools/bench_lora.py [--reps 20] [--steps 28] [--size 1024] [--txt 512] [--skip-image] [--skip-int8] [--out profiles/lora_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "thinkdiff-mlre_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def hip_runtime():
    """The HIP runtime this process already runs on (torch's), for the hipMemcpyDtoDAsync yardstick."""
    with open("/proc/self/maps") as fh:
        for line in fh:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded in this process")


def timed(fn, reps, warm=2):
    """Device-event time of fn() in ms: (median, min, max) over reps after warm warm-up calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return {"median": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--txt", type=int, default=512)
    ap.add_argument("--skip-image", action="store_true")
    ap.add_argument("--skip-int8", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from thinkdiff import _hip
    from thinkdiff.models.flux_prompt import FlowMatchEulerSchedule, FluxPipelineRewritePrompt
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, effective_scalar

    torch.cuda.set_device(0)
    hip = hip_runtime()
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    n_tok, T, N = (a.size // 16) ** 2, a.txt, a.steps
    tr = FluxTransformer2DModel(max_img_tokens=n_tok, max_txt_tokens=T, max_steps=max(32, N)).init_random(1234)
    L = tr._L
    shapes = tr.linear_shapes()
    in_block = lambda n: n.startswith(("transformer_blocks.", "single_transformer_blocks.")) and ".norm" not in n
    targets = [n for n in shapes if in_block(n)]
    elems = sum(shapes[n][0] * shapes[n][1] for n in targets)
    g = torch.Generator(device="cuda").manual_seed(0)
    base = {n: tr.read_param(n) for n in targets}      # the base weights, for the two yardsticks
    scratch = torch.empty(max(shapes[n][0] * shapes[n][1] for n in targets), dtype=torch.bfloat16, device="cuda")
    stream = _hip.stream_ptr

    def make_adapter(rank, seed):
        g.manual_seed(seed)
        sd = {}
        for n in targets:
            Nn, K = shapes[n]
            mod = n[:-len(".weight")]
            sd[mod + ".lora_A.weight"] = (torch.randn(rank, K, generator=g, device="cuda") / K ** 0.5).bfloat16()
            sd[mod + ".lora_B.weight"] = (torch.randn(Nn, rank, generator=g, device="cuda") * 0.02).bfloat16()
        return sd

    def copy_all():      # yardstick 1
        for n in targets:
            hip.hipMemcpyDtoDAsync(scratch.data_ptr(), base[n].data_ptr(), base[n].numel() * 2, stream())

    def torch_merge(adapters, weights):      # yardstick 2 (leaves the merged weights in the arena: the base is loaded back afterwards)
        for n in targets:
            mod = n[:-len(".weight")]
            w = base[n].float()
            for sd, s in zip(adapters, weights):
                w = w + s * (sd[mod + ".lora_B.weight"].float() @ sd[mod + ".lora_A.weight"].float())
            w = w.bfloat16()
            _hip.check(L.td_flux_load_param(tr._h, n.encode(), _hip.ptr(w), w.numel(), stream()))

    def restore_base():
        for n in targets:
            _hip.check(L.td_flux_load_param(tr._h, n.encode(), _hip.ptr(base[n]), base[n].numel(), stream()))
        torch.cuda.synchronize()

    # one image, for the shares and the with / without rates
    image = {}
    if not a.skip_image:
        pe = torch.randn(T, 4096, generator=g, device="cuda").bfloat16()
        pooled = torch.randn(768, generator=g, device="cuda").bfloat16()
        ids = FluxPipelineRewritePrompt._prepare_latent_image_ids(a.size // 16, a.size // 16, "cuda")
        sig = FlowMatchEulerSchedule.sigmas(N, n_tok)
        t_eff = [effective_scalar(float(s) * 1000.0, torch.bfloat16) for s in sig[:-1]]
        lat0 = torch.randn(n_tok, 64, generator=g, device="cuda").bfloat16()

        def one_image():
            tr.set_condition(pe, pooled, ids)
            tr.set_timesteps(t_eff, 3500.0)
            x = lat0.clone()
            tr.denoise(x, sig)
        image["without_adapter_ms"] = timed(one_image, 3, warm=1)

    res = {"metric": "lora", "targets": len(targets), "target_elements": elems, "target_bytes": elems * 2, "cases": {}}
    res["copy_ms"] = timed(copy_all, a.reps)
    res["copy_TBps"] = round(elems * 4 / (res["copy_ms"]["median"] * 1e-3) / 1e12, 3)
    for case, ranks in (("rank16", [16]), ("rank64", [64]), ("rank128", [128]), ("2xrank64", [64, 64])):
        adapters = [make_adapter(r, 10 * r + i) for i, r in enumerate(ranks)]
        names = [f"a{i}" for i in range(len(ranks))]
        weights = [1.0, 0.7][:len(ranks)]
        c = {"ranks": ranks, "operand_share_3072": round(sum((3072 + 3072) * r * 2 for r in ranks) / (3072 * 3072 * 4), 4)}
        c["torch_ms"] = timed(lambda: torch_merge(adapters, weights), max(3, a.reps // 4), warm=1)
        restore_base()
        for nm, sd in zip(names, adapters):
            tr.load_lora_adapter(sd, nm)
        c["bytes_held"] = tr.lora_info()["bytes_held"]
        c["set_adapters_ms"] = timed(lambda: tr.set_adapters(names, weights), a.reps)
        c["copy_again_ms"] = timed(copy_all, a.reps)      # the yardstick next to the measurement, same process state
        c["ratio_to_copy"] = round(c["set_adapters_ms"]["median"] / min(res["copy_ms"]["median"], c["copy_again_ms"]["median"]), 3)
        c["ratio_torch_to_merge"] = round(c["torch_ms"]["median"] / c["set_adapters_ms"]["median"], 2)
        c["merge_TBps_weights_only"] = round(elems * 4 / (c["set_adapters_ms"]["median"] * 1e-3) / 1e12, 3)
        if not a.skip_int8:
            tr.set_precision("int8")
            c["int8_set_adapters_ms"] = timed(lambda: tr.set_adapters(names, weights), max(5, a.reps // 2))
            c["int8_requant_ms"] = timed(lambda: tr.set_precision("int8"), max(5, a.reps // 2))
            tr.set_precision("bf16")
        if not a.skip_image and case == "rank64":
            image["with_adapter_ms"] = timed(one_image, 3, warm=1)
            image["without_adapter_again_ms"] = None
            image["set_adapters_share_of_image"] = round(c["set_adapters_ms"]["median"] / image["with_adapter_ms"]["median"], 5)
        tr.unload_lora()
        if not a.skip_image and case == "rank64":
            image["without_adapter_again_ms"] = timed(one_image, 3, warm=1)
            image["images_per_s"] = {k[:-3]: round(1e3 / v["median"], 4) for k, v in image.items() if isinstance(v, dict)}
        res["cases"][case] = c
        del adapters
        torch.cuda.empty_cache()
    res["image"] = image
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
