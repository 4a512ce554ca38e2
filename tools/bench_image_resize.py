"""The device image resize (td_image_resize_u8) measured three ways; every timed window ends with a device synchronise (or is a pair of device
events), after a warm-up.

  kernels   per-launch device-event time of the resize alone (tables and image already on the device) for 375x500 and 1200x900 to their
            smart_resize sizes and 1024x1024 -> 384x384 BICUBIC, beside the bytes each pass must move (source read once + destination written
            once, per pass) and the resulting ACHIEVED traffic -- bytes the kernel has to move over its time, not a share of any peak.
  builder   host clock of QwenChatFrontend.resolve_requests for 256 image requests (the 500x375 images of tools/bench_precompute_job.py,
            Qwen2-VL-2B-shaped synthetic weights).  --root DIR times the tree at DIR (another checkout of this repository with its library
            built); --time-prep also reports the host stage (the pooled per-image `prep` calls) and the time inside PIL's Image.resize.
  compare   `builder` and tools/bench_precompute_job.py in child processes on this tree and on --parent DIR, alternating, the parent once more
            than this tree so that its own spread is known; writes --out (JSON).

usage: bench_image_resize.py kernels | builder [--root DIR] [--time-prep] [--reps N] | compare --parent DIR [--out FILE] [--job-samples N]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _use_root(root):
    for p in (os.path.join(root, "thinkdiff-mlre_amd"), root):
        sys.path.insert(0, p)


def kernels(args):
    _use_root(ROOT)
    import numpy as np
    import torch
    from thinkdiff import _hip
    from thinkdiff.models.qwen2_vl import smart_resize
    cases = []
    for h, w in ((375, 500), (1200, 900)):
        h2, w2 = smart_resize(h, w, factor=28, min_pixels=56 * 56, max_pixels=28 * 28 * 1280)
        cases.append((f"{h}x{w}->{h2}x{w2} bicubic (smart_resize)", h, w, h2, w2, 3))
    cases.append(("1024x1024->384x384 bicubic", 1024, 1024, 384, 384, 3))
    rng = np.random.default_rng(0)
    out = []
    for name, h, w, h2, w2, f in cases:
        src = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
        dst = torch.empty(h2, w2, 3, dtype=torch.uint8, device="cuda")
        # the wrapper uploads the tables per call; here they go up once so that the events bracket the two kernels alone
        (th, kh), (tv, kv) = _hip.resize_coeffs(w, w2, f), _hip.resize_coeffs(h, h2, f)
        dh, dv = torch.from_numpy(np.array(th)).cuda(), torch.from_numpy(np.array(tv)).cuda()      # copies: the cached tables are read-only
        tmp = torch.empty(h * w2 * 3, dtype=torch.uint8, device="cuda")
        import ctypes
        vp = ctypes.c_void_p

        def launch():
            _hip.check(_hip.lib().td_image_resize_u8(_hip.ptr(src), h, w, 3, _hip.ptr(dst), h2, w2, 3, vp(dh.data_ptr()), vp(dh.data_ptr() + 8 * w2), kh,
                                                     vp(dv.data_ptr()), vp(dv.data_ptr() + 8 * h2), kv, _hip.ptr(tmp), _hip.stream_ptr()))
        for _ in range(10):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        times.sort()
        med = times[len(times) // 2]
        b_h, b_v = 3 * (h * w + h * w2), 3 * (h * w2 + h2 * w2)
        # and the whole wrapper call (host table lookup + table upload + both launches), host clock with a synchronise inside
        for _ in range(5):
            _hip.image_resize_u8(src, h2, w2, f, out=dst)
        torch.cuda.synchronize()
        wt = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _hip.image_resize_u8(src, h2, w2, f, out=dst)
            torch.cuda.synchronize()
            wt.append(time.perf_counter() - t0)
        wt.sort()
        out.append({"case": name, "ksize_h": kh, "ksize_v": kv, "device_us_median": med * 1e6, "device_us_min": times[0] * 1e6, "device_us_max": times[-1] * 1e6,
                    "bytes_horizontal_pass": b_h, "bytes_vertical_pass": b_v, "achieved_GB_per_s": (b_h + b_v) / med / 1e9,
                    "wrapper_call_host_us_median": wt[len(wt) // 2] * 1e6, "reps": args.reps})
        print(json.dumps(out[-1]), flush=True)
    return out


def builder(args):
    root = os.path.abspath(args.root or ROOT)
    _use_root(root)
    import numpy as np
    import torch
    from PIL import Image
    from thinkdiff.common.config import Node
    from thinkdiff.models import providers
    from thinkdiff.models.mllama_vllm_generate_1 import MllamaVllmGenerate_1
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig
    import thinkdiff
    assert os.path.abspath(thinkdiff.__file__).startswith(root), (thinkdiff.__file__, root)
    tc = Qwen2VLTextConfig(hidden_size=1536, num_hidden_layers=28, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                           vocab_size=151936, tie_word_embeddings=True)
    m = MllamaVllmGenerate_1(tc, vllm_config={"max_model_len": 2048, "max_tokens": 8, "min_tokens": 1, "ignore_eos": False, "max_num_seqs": 16})
    providers.load_lvlm_frontend(Node({"synthetic": True, "seed": 0, "synthetic_max_image_tokens": 320}), m, "cuda")
    base = np.random.default_rng(0).integers(0, 256, (24, 32, 3), dtype=np.uint8)
    n = 256
    imgs = [Image.fromarray(np.roll(base, k, axis=1)).resize((500, 375), Image.BICUBIC) for k in range(n)]      # bench_precompute_job.py's images
    reqs = m.chat_requests(["Describe the image in one sentence."] * n, imgs)
    stage = {"prep_stage_s": 0.0, "pil_resize_thread_s": 0.0, "pil_resize_calls": 0}
    if args.time_prep:
        import threading
        from concurrent.futures import ThreadPoolExecutor
        lock = threading.Lock()
        pool_map, pil_resize = ThreadPoolExecutor.map, Image.Image.resize

        def timed_map(self, fn, *its, **kw):          # the frontend's `list(pool.map(prep, images))`: the iterator is drained inside the window
            t0 = time.perf_counter()
            r = list(pool_map(self, fn, *its, **kw))
            stage["prep_stage_s"] += time.perf_counter() - t0
            return iter(r)

        def timed_resize(self, *a, **kw):
            t0 = time.perf_counter()
            r = pil_resize(self, *a, **kw)
            dt = time.perf_counter() - t0
            with lock:
                stage["pil_resize_thread_s"] += dt
                stage["pil_resize_calls"] += 1
            return r
        ThreadPoolExecutor.map, Image.Image.resize = timed_map, timed_resize
    for _ in range(2):
        m.resolve_requests(reqs)
    torch.cuda.synchronize()
    for k in stage:
        stage[k] = 0
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.resolve_requests(reqs)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res = {"root": root, "requests": n, "reps": args.reps, "resolve_requests_s": times, "median_s": sorted(times)[len(times) // 2], "min_s": min(times)}
    if args.time_prep:
        res.update({"prep_stage_s_per_call": stage["prep_stage_s"] / args.reps, "pil_resize_thread_s_per_call": stage["pil_resize_thread_s"] / args.reps,
                    "pil_resize_calls_per_call": stage["pil_resize_calls"] / args.reps})
    print("RESULT " + json.dumps(res), flush=True)
    return res


def _child(argv, timeout):
    p = subprocess.run([sys.executable] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    if p.returncode != 0:
        print(p.stdout[-4000:])
        raise SystemExit(f"child {argv} ended with status {p.returncode}: nothing more is started")
    return p.stdout


def compare(args):
    parent = os.path.abspath(args.parent)
    trees = [("parent", parent), ("this", ROOT), ("parent", parent), ("this", ROOT), ("parent", parent)]
    res = {"builder": [], "job": []}
    for name, root in trees:
        out = _child([os.path.abspath(__file__), "builder", "--root", root, "--reps", str(args.reps)] + (["--time-prep"] if name == "parent" else []), 400)
        r = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
        r["tree"] = name
        res["builder"].append(r)
        print(json.dumps(r), flush=True)
    if args.job_samples > 0:
        import re
        for name, root in trees:
            out = _child([os.path.join(root, "tools", "bench_precompute_job.py"), str(args.job_samples), str(min(512, args.job_samples))], 500)
            mm = re.search(r"precompute job: (\d+) samples in ([0-9.]+) s = ([0-9.]+) samples/s", out)
            r = {"tree": name, "samples": int(mm.group(1)), "seconds": float(mm.group(2)), "samples_per_s": float(mm.group(3))}
            res["job"].append(r)
            print(json.dumps(r), flush=True)

    def spread(key, rows, tree):
        v = [r[key] for r in rows if r["tree"] == tree]
        return {"values": v, "min": min(v), "max": max(v), "mean": sum(v) / len(v)} if v else None
    res["summary"] = {"builder_median_s": {t: spread("median_s", res["builder"], t) for t in ("parent", "this")},
                      "job_samples_per_s": {t: spread("samples_per_s", res["job"], t) for t in ("parent", "this")}}
    print(json.dumps(res["summary"], indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "builder", "compare"])
    ap.add_argument("--root")
    ap.add_argument("--parent")
    ap.add_argument("--time-prep", action="store_true")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--out")
    ap.add_argument("--job-samples", type=int, default=1024)
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 50 if a.what == "kernels" else 5
    if a.what == "kernels":
        r = kernels(a)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump({"kernels": r}, fh, indent=1)
    elif a.what == "builder":
        builder(a)
    else:
        if not a.parent:
            raise SystemExit("compare needs --parent DIR (a checkout of the parent commit with its library built)")
        compare(a)
