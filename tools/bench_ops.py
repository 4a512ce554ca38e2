"""Micro-benchmarks of the individual HIP ops on the GPU box (not the headline bench)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thinkdiff-mlre_amd"))
from thinkdiff import _hip  # noqa: E402


def timeit(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def bench_gemm():
    shapes = [  # (M, N, K) of the FLUX.1-dev cfg-2 step
        (4096, 9216, 3072), (4096, 3072, 3072), (4096, 12288, 3072), (4096, 3072, 12288),
        (4289, 21504, 3072), (4289, 3072, 15360), (193, 9216, 3072), (193, 12288, 3072),
        (4096, 4096, 4096), (8192, 8192, 8192), (28, 18432, 3072),
    ]
    for M, N, K in shapes:
        x = torch.randn(M, K, device="cuda").bfloat16()
        w = (torch.randn(N, K, device="cuda") * 0.02).bfloat16()
        b = torch.randn(N, device="cuda").bfloat16()
        out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        ms = timeit(lambda: _hip.linear(x, w, b, out=out))
        tf = 2.0 * M * N * K / ms / 1e9
        ref_ms = timeit(lambda: torch.nn.functional.linear(x, w, b))
        print(f"gemm M={M:5d} N={N:5d} K={K:5d}: {ms:8.3f} ms  {tf:7.1f} TF/s   (hipBLASLt via torch: {ref_ms:8.3f} ms {2.0*M*N*K/ref_ms/1e9:7.1f} TF/s)", flush=True)


def bench_gemmcfg():
    """256x256 vs 288x192 tiles on the FLUX shapes (grouped = image + 193 text rows in one launch)."""
    shapes = [(4096, 193, 9216, 3072), (4096, 193, 3072, 3072), (4096, 193, 12288, 3072), (4096, 193, 3072, 12288),
              (4289, 0, 21504, 3072), (4289, 0, 3072, 15360)]
    for M0, M1, N, K in shapes:
        x0 = torch.randn(M0, K, device="cuda").bfloat16(); w0 = (torch.randn(N, K, device="cuda") * 0.02).bfloat16()
        b0 = torch.randn(N, device="cuda").bfloat16(); y0 = torch.empty(M0, N, device="cuda", dtype=torch.bfloat16)
        if M1:
            x1 = torch.randn(M1, K, device="cuda").bfloat16(); w1 = (torch.randn(N, K, device="cuda") * 0.02).bfloat16()
            y1 = torch.empty(M1, N, device="cuda", dtype=torch.bfloat16)
        else:
            x1 = w1 = y1 = None
        fl = 2.0 * (M0 + M1) * N * K
        cfgs = (0, 3)
        best = {c: 1e9 for c in cfgs}
        for rnd in range(5):   # interleaved rounds in one process (guide rule 24)
            for cfg in cfgs:
                ms = timeit(lambda: _hip.linear_grouped2(x0, w0, b0, y0, x1, w1, b0 if M1 else None, y1, tile_cfg=cfg), iters=10, warmup=2)
                best[cfg] = min(best[cfg], ms)
        print(f"M={M0}+{M1} N={N} K={K}:  " + "   ".join(f"cfg{c}: {best[c]:7.3f} ms {fl/best[c]/1e9:7.1f} TF/s" for c in cfgs), flush=True)


def bench_gemmtile():
    """CU time of one tile of the 256x256 (cfg 0) and the 288x192 (cfg 3) shape per operand type: M = 4289, N = 3072 is ONE round of either (204 /
    240 tiles on 256 CUs), so a launch's time is its tile's time.  Cold weights (pool cycling), interleaved rounds, K swept; the least-squares line
    time = c0 + c1 * k-tiles (a k-tile = 128 operand bytes per row: 64 bf16 / 128 8-bit elements) gives the constants of the shared-chip tile
    table in csrc/gemm_bf16.hip (td_gemm_plan), and tiles x time is the CU time the launch takes from a chip that other kernels keep full."""
    M, N = 4289, 3072
    tiles = {0: 204, 3: 240}
    for kind in ("bf16", "int8", "fp8"):
        esz = 2 if kind == "bf16" else 1
        pts = {0: [], 3: []}
        for kt in (96, 144, 192, 240):
            K = kt * 128 // esz
            x = torch.randn(M, K, device="cuda").bfloat16()
            npool = max(2, int(0.8e9 // (N * K * esz)))
            pool = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(npool)]
            b = torch.randn(N, device="cuda").bfloat16()
            y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            st = {"i": 0}
            if kind == "bf16":
                def f(cfg):
                    st["i"] = (st["i"] + 1) % npool
                    _hip.linear_grouped2(x, pool[st["i"]], b, y, None, None, None, None, tile_cfg=cfg)
            else:
                quant, lin = (_hip.quant_rows_int8, _hip.linear_int8) if kind == "int8" else (_hip.quant_rows_fp8, _hip.linear_fp8)
                qpool = [quant(w) for w in pool]
                xq, xs = quant(x)
                del pool
                def f(cfg):
                    st["i"] = (st["i"] + 1) % npool
                    wq, ws = qpool[st["i"]]
                    lin(xq, xs, wq, ws, b, out=y, tile_cfg=cfg)
            best = {0: 1e9, 3: 1e9}
            for rnd in range(5):
                for cfg in (0, 3):
                    best[cfg] = min(best[cfg], timeit(lambda: f(cfg), iters=10, warmup=2))
            for cfg in (0, 3):
                pts[cfg].append((kt, best[cfg] * 1e3))
            print(f"{kind} M={M} N={N} K={K} ({kt} k-tiles): " + "   ".join(
                f"cfg{c}: {best[c]*1e3:7.1f} us x {tiles[c]} tiles = {best[c]*tiles[c]:6.2f} CU.ms" for c in (0, 3)) +
                f"   cfg0 / cfg3 CU time {best[0]*tiles[0]/(best[3]*tiles[3]):.3f}", flush=True)
        for cfg in (0, 3):
            n = len(pts[cfg]); sx = sum(p[0] for p in pts[cfg]); sy = sum(p[1] for p in pts[cfg])
            sxx = sum(p[0] * p[0] for p in pts[cfg]); sxy = sum(p[0] * p[1] for p in pts[cfg])
            c1 = (n * sxy - sx * sy) / (n * sxx - sx * sx); c0 = (sy - c1 * sx) / n
            print(f"{kind} cfg{cfg}: c0 = {c0:6.2f} us per tile, c1 = {c1:6.4f} us per k-tile", flush=True)


def bench_gemmfp8():
    """fp8 (e4m3, v_mfma_scale 16x16x128) and int8 (v_mfma_i32_16x16x64_i8) vs bf16 GEMM on the FLUX shapes, cold weights (pool cycling),
    interleaved; plus the sustained FLUX-step mix per operand type (3 s windows, alternating)."""
    ops = {}
    for name, M, N, K in [("single_in", 4289, 21504, 3072), ("qkv", 4289, 9216, 3072), ("ff1", 4289, 12288, 3072), ("attn_out", 4289, 3072, 3072),
                          ("ff2", 4289, 3072, 12288), ("single_out", 4289, 3072, 15360)]:
        x = torch.randn(M, K, device="cuda").bfloat16()
        npool = max(2, int(0.8e9 // (N * K * 2)))
        pool = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(npool)]
        qpool = [_hip.quant_rows_fp8(w) for w in pool]
        ipool = [_hip.quant_rows_int8(w) for w in pool]
        xq, xs = _hip.quant_rows_fp8(x)
        xi, xis = _hip.quant_rows_int8(x)
        b = torch.randn(N, device="cuda").bfloat16()
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        fl = 2.0 * M * N * K
        st = {"i": 0}
        def f_bf16(x=x, pool=pool, b=b, y=y, st=st, npool=npool):
            st["i"] = (st["i"] + 1) % npool
            _hip.linear(x, pool[st["i"]], b, out=y)
        def f_fp8(xq=xq, xs=xs, qpool=qpool, b=b, y=y, st=st, npool=npool):
            st["i"] = (st["i"] + 1) % npool
            wq, ws = qpool[st["i"]]
            _hip.linear_fp8(xq, xs, wq, ws, b, out=y)
        def f_int8(xi=xi, xis=xis, ipool=ipool, b=b, y=y, st=st, npool=npool):
            st["i"] = (st["i"] + 1) % npool
            wq, ws = ipool[st["i"]]
            _hip.linear_int8(xi, xis, wq, ws, b, out=y)
        fns = {"bf16": f_bf16, "fp8": f_fp8, "int8": f_int8}
        ops[name] = (fns, fl)
        best = {k: 1e9 for k in fns}
        for rnd in range(4):
            for k, f in fns.items():
                best[k] = min(best[k], timeit(f, iters=10, warmup=2))
        print(f"{name:10s} M={M} N={N} K={K}: " + "   ".join(f"{k} {best[k]:7.3f} ms {fl/best[k]/1e9:7.1f} TF/s" for k in fns) +
              f"   fp8 x{best['bf16']/best['fp8']:.2f}  int8 x{best['bf16']/best['int8']:.2f}", flush=True)
    seq = [("qkv", 1), ("attn_out", 1), ("ff1", 1), ("ff2", 1), ("single_in", 2), ("single_out", 2)]
    fl_seq = sum(ops[n][1] * k for n, k in seq)
    res = {k: [] for k in ("bf16", "fp8", "int8")}
    for rnd in range(2):
        for which in res:
            def run_seq():
                for n, k in seq:
                    for _ in range(k):
                        ops[n][0][which]()
            run_seq(); torch.cuda.synchronize()
            t0 = time.perf_counter(); n_it = 0
            while time.perf_counter() - t0 < 3.0:
                for _ in range(10):
                    run_seq()
                torch.cuda.synchronize(); n_it += 10
            res[which].append(fl_seq * n_it / (time.perf_counter() - t0) / 1e12)
    print("sustained FLUX-step GEMM mix (3 s windows): " + " | ".join(f"{k} " + " ".join(f"{v:6.0f}" for v in vs) + " TF/s" for k, vs in res.items()), flush=True)


def bench_gemmprobe():
    """Where a block GEMM's time goes: the whole launch, the k-loop alone (TD_GEMM_PROBE=1: no epilogue) and the prologue + epilogue alone
    (TD_GEMM_PROBE=2: one k-tile), bf16 and int8, GELU epilogue, cold weights, tail split off and on; with the tail split off, the bf16 launch both
    as one tile per workgroup (TD_GEMM_DRAIN=0) and as the persistent walk with deferred stores (the int8 kernels have no such form)."""
    for name, M, N, K in [("ff1", 4289, 12288, 3072), ("qkv", 4289, 9216, 3072), ("single_in", 4289, 21504, 3072), ("ff1 T=258", 4354, 12288, 3072)]:
        x = torch.randn(M, K, device="cuda").bfloat16()
        npool = max(2, int(0.8e9 // (N * K * 2)))
        pool = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(npool)]
        ipool = [_hip.quant_rows_int8(w) for w in pool]
        xi, xis = _hip.quant_rows_int8(x)
        b = torch.randn(N, device="cuda").bfloat16()
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        st = {"i": 0}
        def f_bf16():
            st["i"] = (st["i"] + 1) % npool
            _hip.linear_grouped2(x, pool[st["i"]], b, y, None, None, None, None, act=_hip.ACT_GELU_TANH, tile_cfg=0)
        def f_int8():
            st["i"] = (st["i"] + 1) % npool
            wq, ws = ipool[st["i"]]
            _hip.linear_int8(xi, xis, wq, ws, b, act=_hip.ACT_GELU_TANH, out=y, tile_cfg=0)
        for tail, drain in (("off", "off"), ("off", "on"), ("on", "off")):
            if tail == "off":
                os.environ.pop("TD_GEMM_TAIL", None)
            else:
                os.environ["TD_GEMM_TAIL"] = "auto"
            if drain == "off":
                os.environ["TD_GEMM_DRAIN"] = "0"
            else:
                os.environ["TD_GEMM_DRAIN"] = "1"
            row = []
            for kind, f in (("bf16", f_bf16), ("int8", f_int8)):
                t = {}
                for probe in ("0", "1", "2"):
                    os.environ["TD_GEMM_PROBE"] = probe
                    t[probe] = min(timeit(f, iters=10, warmup=2) for _ in range(3))
                os.environ.pop("TD_GEMM_PROBE")
                row.append(f"{kind}: whole {t['0']*1e3:6.1f} us  k-loop only {t['1']*1e3:6.1f}  1 k-tile + epilogue {t['2']*1e3:6.1f}")
            print(f"{name:10s} M={M} N={N} K={K} tail split {tail:3s} drain {drain:3s} | " + " | ".join(row), flush=True)
        os.environ.pop("TD_GEMM_DRAIN", None)
        del pool, ipool


def bench_gemmepi():
    """The six block GEMMs of a FLUX step with their real epilogues (bias / GELU / gate + residual / split output), cold weights."""
    S = 4289
    cases = [("qkv   bias", 9216, 3072, "bias"), ("out   gate+res", 3072, 3072, "gr"), ("ff1   gelu", 12288, 3072, "gelu"),
             ("ff2   gate+res", 3072, 12288, "gr"), ("W1    split+gelu", 21504, 3072, "split"), ("W2    gate+res", 3072, 15360, "gr")]
    tot = 0.0
    for name, N, K, kind in cases:
        x = torch.randn(S, K, device="cuda").bfloat16()
        npool = max(2, int(1.2e9 // (N * K * 2)))
        pool = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(npool)]
        b = torch.randn(N, device="cuda").bfloat16()
        g = torch.randn(N, device="cuda").bfloat16()
        y = torch.empty(S, N, device="cuda", dtype=torch.bfloat16)
        r = torch.randn(S, N, device="cuda").bfloat16() if kind == "gr" else None
        y0 = torch.empty(S, 9216, device="cuda", dtype=torch.bfloat16) if kind == "split" else None
        y1 = torch.empty(S, 15360, device="cuda", dtype=torch.bfloat16)[:, 3072:] if kind == "split" else None
        st = {"i": 0}
        def f():
            st["i"] = (st["i"] + 1) % npool
            w = pool[st["i"]]
            if kind == "bias": _hip.linear(x, w, b, out=y)
            elif kind == "gelu": _hip.linear(x, w, b, act=_hip.ACT_GELU_TANH, out=y)
            elif kind == "gr": _hip.linear(x, w, b, gate=g, res=r, out=r)
            else: _hip.linear_split(x, w, b, y0, _hip.ACT_NONE, y1, _hip.ACT_GELU_TANH, 9216)
        best = min(timeit(f, iters=10, warmup=2) for _ in range(4))
        tot += best
        print(f"{name:18s} N={N:5d} K={K:5d}: {best*1e3:7.1f} us  {2.0*S*N*K/best/1e9:7.1f} TF/s", flush=True)
        del pool
    print(f"sum {tot:.3f} ms")


def bench_gemmsmall():
    """Mid-M Linears (encoders, towers, short prefills): 256x256 tiles (cfg 0) vs 256x64 tiles (cfg 1) vs 32x256 (cfg 2, M <= 32)."""
    for M, N, K in [(128, 24576, 4096), (128, 20480, 4096), (128, 4096, 10240), (300, 4608, 3584), (300, 37888, 3584), (300, 3584, 18944),
                    (257, 6144, 1408), (257, 1408, 6144), (77, 3072, 768), (512, 4096, 4096), (1024, 3840, 1280)]:
        x = torch.randn(M, K, device="cuda").bfloat16()
        pool = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(max(2, int(6e8 // (N * K * 2))))]
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        st = {"i": 0}
        res = {}
        for cfg in (0, 1):
            def f():
                st["i"] = (st["i"] + 1) % len(pool)
                _hip.linear_grouped2(x, pool[st["i"]], None, y, None, None, None, None, tile_cfg=cfg)
            res[cfg] = min(timeit(f, iters=10, warmup=2) for _ in range(3))
        print(f"M={M} N={N} K={K}: cfg0 {res[0]*1e3:7.1f} us   cfg1 {res[1]*1e3:7.1f} us   weights {N*K*2/1e6:.0f} MB -> {N*K*2/min(res.values())/1e6:.0f} GB/s", flush=True)
        del pool


def bench_batch3():
    """Would true batching of 3 images (M = 3 x 4289 rows per GEMM, attention batch 3) beat 3 separate launches?  Cold weights."""
    S = 4289
    tot1 = tot3 = 0.0
    for name, N, K, count in [("qkv", 9216, 3072, 19), ("out", 3072, 3072, 19), ("ff1", 12288, 3072, 19), ("ff2", 3072, 12288, 19),
                              ("W1", 21504, 3072, 38), ("W2", 3072, 15360, 38)]:
        x1 = torch.randn(S, K, device="cuda").bfloat16()
        x3 = torch.randn(3 * S, K, device="cuda").bfloat16()
        npool = max(2, int(1.2e9 // (N * K * 2)))
        pool = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(npool)]
        b = torch.randn(N, device="cuda").bfloat16()
        y1 = torch.empty(S, N, device="cuda", dtype=torch.bfloat16)
        y3 = torch.empty(3 * S, N, device="cuda", dtype=torch.bfloat16)
        st = {"i": 0}
        def f1():
            st["i"] = (st["i"] + 1) % npool
            for _ in range(3):
                _hip.linear(x1, pool[st["i"]], b, out=y1)
        def f3():
            st["i"] = (st["i"] + 1) % npool
            _hip.linear(x3, pool[st["i"]], b, out=y3)
        t1 = min(timeit(f1, iters=6, warmup=2) for _ in range(3))
        t3 = min(timeit(f3, iters=6, warmup=2) for _ in range(3))
        fl = 2.0 * 3 * S * N * K
        print(f"{name:4s} N={N:5d} K={K:5d}: 3 launches {t1*1e3:7.1f} us ({fl/t1/1e9:6.0f} TF/s)   one M=3S launch {t3*1e3:7.1f} us ({fl/t3/1e9:6.0f} TF/s)   x{t1/t3:.3f}", flush=True)
        tot1 += t1 * count; tot3 += t3 * count
        del pool
    H = 24
    q1 = torch.randn(1, S, 3 * H * 128, device="cuda").bfloat16()
    q3 = torch.randn(3, S, 3 * H * 128, device="cuda").bfloat16()
    o1 = torch.empty(1, S, H * 128, device="cuda", dtype=torch.bfloat16)
    o3 = torch.empty(3, S, H * 128, device="cuda", dtype=torch.bfloat16)
    W = H * 128
    def a1():
        for _ in range(3):
            _hip.attention(q1[:, :, :W], q1[:, :, W:2 * W], q1[:, :, 2 * W:], o1, H, H)
    def a3():
        _hip.attention(q3[:, :, :W], q3[:, :, W:2 * W], q3[:, :, 2 * W:], o3, H, H)
    t1 = min(timeit(a1, iters=6, warmup=2) for _ in range(3))
    t3 = min(timeit(a3, iters=6, warmup=2) for _ in range(3))
    fl = 3 * 4.0 * S * S * H * 128
    print(f"attention: 3 launches {t1*1e3:7.1f} us ({fl/t1/1e9:6.0f} TF/s)   batch-3 launch {t3*1e3:7.1f} us ({fl/t3/1e9:6.0f} TF/s)   x{t1/t3:.3f}", flush=True)
    tot1 += t1 * 57; tot3 += t3 * 57
    print(f"per step (3 images): separate {tot1:.1f} ms, batched {tot3:.1f} ms  -> x{tot1/tot3:.3f}; per image per 28 steps {tot1*28/3:.0f} vs {tot3*28/3:.0f} ms")


def bench_attn1():
    """Joint attention at the FLUX shape, cold inputs (pool cycling)."""
    S, H = 4289, 24
    W = H * 128
    pool = [torch.randn(1, S, 3 * W, device="cuda").bfloat16() for _ in range(6)]
    o = torch.empty(1, S, W, device="cuda", dtype=torch.bfloat16)
    st = {"i": 0}
    def f():
        st["i"] = (st["i"] + 1) % len(pool)
        q = pool[st["i"]]
        _hip.attention(q[:, :, :W], q[:, :, W:2 * W], q[:, :, 2 * W:], o, H, H)
    ms = min(timeit(f, iters=20, warmup=3) for _ in range(6))
    print(f"attention S={S} H={H}: {ms*1e3:6.1f} us  {4.0*S*S*H*128/ms/1e9:6.0f} TF/s")


def bench_gemmcold():
    """Tile/pipeline variants with L3-warm weights (one W re-used) vs cold weights (cycling a 1 GB pool, as in
    the real denoise loop where every layer's weights stream from HBM).  Interleaved rounds, best-of."""
    import sys
    cfgs = [int(c) for c in os.environ.get("TD_CFGS", "0,3").split(",")]
    for M, N, K in [(4289, 21504, 3072), (4289, 3072, 15360), (4289, 9216, 3072), (4289, 12288, 3072), (4289, 3072, 12288)]:
        x = torch.randn(M, K, device="cuda").bfloat16()
        pool = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(max(2, int(1.2e9 // (N * K * 2))))]
        b = torch.randn(N, device="cuda").bfloat16()
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        fl = 2.0 * M * N * K
        state = {"i": 0}
        def run(cfg, cold):
            def f():
                if cold:
                    state["i"] = (state["i"] + 1) % len(pool)
                _hip.linear_grouped2(x, pool[state["i"] if cold else 0], b, y, None, None, None, None, tile_cfg=cfg)
            return f
        best = {(c, k): 1e9 for c in cfgs for k in (0, 1)}
        for _ in range(4):
            for c in cfgs:
                for k in (0, 1):
                    best[(c, k)] = min(best[(c, k)], timeit(run(c, k), iters=16, warmup=2))
        print(f"M={M} N={N} K={K}: " + " | ".join(f"cfg{c} warm {fl/best[(c,0)]/1e9:6.0f} cold {fl/best[(c,1)]/1e9:6.0f}" for c in cfgs) + " TF/s", flush=True)


def bench_attn():
    """Joint attention, in-process interleaved A/B of the kernel structures (variant 0 shipped / 1 one workgroup per item /
    2 persistent without the XCD range order), cold inputs (pool cycling)."""
    names = {0: "shipped", 1: "wg-per-item", 0x800: "shipped-prescaled", 0x801: "wg-per-item-prescaled"}
    for S, H in [(4289, 24), (4354, 24)]:
        W = H * 128
        pool = [torch.randn(1, S, 3 * W, device="cuda").bfloat16() for _ in range(6)]
        out = torch.empty(1, S, W, device="cuda", dtype=torch.bfloat16)
        st = {"i": 0}
        def f():
            st["i"] = (st["i"] + 1) % len(pool)
            q = pool[st["i"]]
            _hip.attention(q[:, :, :W], q[:, :, W:2 * W], q[:, :, 2 * W:], out, H, H)
        best = {v: 1e9 for v in names}
        for _ in range(5):
            for var in names:
                _hip.lib().td_attention_set_variant(var)
                best[var] = min(best[var], timeit(f, iters=10, warmup=2))
        _hip.lib().td_attention_set_variant(0)
        fl = 4.0 * S * S * H * 128
        print(f"attn S={S} H={H}: " + "   ".join(f"{names[v]} {best[v]*1e3:6.1f} us {fl/best[v]/1e9:6.0f} TF/s" for v in names), flush=True)


def bench_attn_m16():
    """The score-bound joint attention (td_attention_joint_prescaled_bf16, the form the FLUX engine runs): its 16x16x32 MFMA body against the 32x32x16
    body (variant bit 0x400), persistent form and one workgroup per item (variant 1), arms alternated in one process on cold random inputs (pool
    cycling; q and k uniform in +-0.25 so that the bound of 8 octaves holds).  Median and minimum per arm over the alternations."""
    import statistics
    arms = {"streamk m32": 0x400, "streamk m16": 0, "per-item m32": 0x401, "per-item m16": 1}
    S, H = 4289, 24
    W = H * 128
    pool = []
    for _ in range(6):
        t = torch.randn(S, 3 * W, device="cuda")
        t[:, :2 * W] = torch.rand(S, 2 * W, device="cuda") * 0.5 - 0.25
        pool.append(t.bfloat16())
    out = torch.empty(S, W, device="cuda", dtype=torch.bfloat16)
    st = {"i": 0}
    def f():
        st["i"] = (st["i"] + 1) % len(pool)
        q = pool[st["i"]]
        _hip.attention_joint_prescaled(q[:, :W], q[:, W:2 * W], q[:, 2 * W:], out, H, 8.0)
    res = {a: [] for a in arms}
    for _ in range(9):
        for a, var in arms.items():
            _hip.lib().td_attention_set_variant(var)
            res[a].append(timeit(f, iters=10, warmup=2))
    _hip.lib().td_attention_set_variant(0)
    fl = 4.0 * S * S * H * 128
    for a, v in res.items():
        print(f"attn_m16 S={S} H={H} {a}: median {statistics.median(v)*1e3:6.1f} us min {min(v)*1e3:6.1f} us max {max(v)*1e3:6.1f} us  {fl/min(v)/1e9:6.0f} TF/s", flush=True)


def bench_attn8():
    """The 8-bit joint attention (pack + attention kernels together) against the shipped bf16 kernel, interleaved, cold inputs."""
    for S, H in [(4289, 24), (4354, 24)]:
        W = H * 128
        pool = [torch.randn(S, 3 * W, device="cuda").bfloat16() for _ in range(6)]
        out = torch.empty(S, W, device="cuda", dtype=torch.bfloat16)
        L = _hip.lib()
        L.td_attention_fp8_workspace_bytes.restype = __import__("ctypes").c_size_t
        ws = torch.empty(int(L.td_attention_fp8_workspace_bytes(S, S, H)), dtype=torch.uint8, device="cuda")
        st = {"i": 0}
        def f16():
            st["i"] = (st["i"] + 1) % len(pool)
            q = pool[st["i"]][None]
            _hip.attention(q[:, :, :W], q[:, :, W:2 * W], q[:, :, 2 * W:], out[None], H, H)
        def f8():
            st["i"] = (st["i"] + 1) % len(pool)
            q = pool[st["i"]]
            _hip.attention_fp8(q[:, :W], q[:, W:2 * W], q[:, 2 * W:], out, H, workspace=ws)
        best = {"bf16": 1e9, "fp8": 1e9, "fp8-4wave": 1e9, "fp8-exp2": 1e9, "fp8-4wave-exp2": 1e9}
        for _ in range(5):
            best["bf16"] = min(best["bf16"], timeit(f16, iters=10, warmup=2))
            best["fp8"] = min(best["fp8"], timeit(f8, iters=10, warmup=2))
            for var, name in ((1, "fp8-4wave"), (2, "fp8-exp2"), (3, "fp8-4wave-exp2")):
                L.td_attention_set_variant(var)
                best[name] = min(best[name], timeit(f8, iters=10, warmup=2))
            L.td_attention_set_variant(0)
        fl = 4.0 * S * S * H * 128
        print(f"attn8 S={S} H={H}: " + "   ".join(f"{k} {v*1e3:6.1f} us {fl/v/1e9:6.0f} TF/s" for k, v in best.items()), flush=True)


def bench_pack8():
    """Where the 8-bit attention's pack pass spends its time: the fused form (QK-RMSNorm + RoPE inside the pass, as the engine runs it) with its
    q / k / v sections switched off in turn (TD_PACK_PROBE; the attention kernel then runs on stale operands -- durations only)."""
    S, H = 4354, 24
    W = H * 128
    pool = [torch.randn(S, 3 * W, device="cuda").bfloat16() for _ in range(6)]
    out = torch.empty(S, W, device="cuda", dtype=torch.bfloat16)
    cos, sin = torch.rand(S, 128, device="cuda"), torch.rand(S, 128, device="cuda")
    wq, wk = torch.ones(128, device="cuda").bfloat16(), torch.ones(128, device="cuda").bfloat16()
    L = _hip.lib()
    L.td_attention_fp8_workspace_bytes.restype = __import__("ctypes").c_size_t
    ws = torch.empty(int(L.td_attention_fp8_workspace_bytes(S, S, H)), dtype=torch.uint8, device="cuda")
    st = {"i": 0}
    def f():
        st["i"] = (st["i"] + 1) % len(pool)
        _hip.attention_fp8_qk_rope(pool[st["i"]], out, H, cos, sin, split=258, wqA=wq, wkA=wk, wqB=wq, wkB=wk, workspace=ws)
    res = {}
    for _ in range(3):
        for probe in (0, 1, 2, 4, 7):
            os.environ["TD_PACK_PROBE"] = str(probe)
            res[probe] = min(res.get(probe, 1e9), timeit(f, iters=10, warmup=2))
    os.environ.pop("TD_PACK_PROBE")
    base = res[7]
    print(f"pack + attention S={S}: all {res[0]*1e3:.1f} us; attention alone (pack sections off) {base*1e3:.1f}; pack {1e3*(res[0]-base):.1f} = "
          f"v {1e3*(res[0]-res[1]):.1f} + k {1e3*(res[0]-res[2]):.1f} + q {1e3*(res[0]-res[4]):.1f} (+ fixed {1e3*(res[1]+res[2]+res[4]-2*res[0]-base):.1f})", flush=True)


def bench_norm():
    """td_norm_rows_kernel<6> at the denoise loop's shape: LayerNorm + adaLN modulate of the joint [text | image] rows (S = 4354, D = 3072), bf16 out and
    int8 out, rotating over six inputs larger than the caches.  Rows per wave come from TD_NORM_ROWS_PER_WAVE (read once per process)."""
    S, D = 4354, 3072
    pool = [torch.randn(S, D, device="cuda").bfloat16() for _ in range(6)]
    mods = [torch.randn(D, device="cuda").bfloat16() * 0.1 for _ in range(4)]
    out = torch.empty(S, D, device="cuda", dtype=torch.bfloat16)
    st = {"i": 0}
    def f():
        st["i"] = (st["i"] + 1) % len(pool)
        _hip.norm_rows(pool[st["i"]], out=out, eps=1e-6, split=258, shiftA=mods[0], scaleA=mods[1], shiftB=mods[2], scaleB=mods[3])
    def g():
        st["i"] = (st["i"] + 1) % len(pool)
        _hip.norm_rows_quant_fp8(pool[st["i"]], eps=1e-6, split=258, shiftA=mods[0], scaleA=mods[1], shiftB=mods[2], scaleB=mods[3])
    best = min(timeit(f, iters=50, warmup=5) for _ in range(3))
    bq = min(timeit(g, iters=50, warmup=5) for _ in range(3))
    print(f"norm rows S={S} D={D} rows/wave={os.environ.get('TD_NORM_ROWS_PER_WAVE', 'auto')}: bf16 out {best*1e3:.1f} us = {2*S*D*2/best/1e9:.2f} TB/s; "
          f"8-bit out {bq*1e3:.1f} us", flush=True)


def bench_blockcache():
    """The first-block cache's two kernels at the 1024^2 shape (4096 image rows of a [4608, 3072] joint buffer; and 8192 rows: Kontext) against
    hipMemcpyAsync (torch's device-to-device copy_) of the SAME byte count in the same process, rotating over operand sets larger than the caches.
    head: reads h1, h0, r_prev, writes r (4 x rows x D x 2 bytes) + the partial-sum finish launch; tail: reads a, b, writes out (3 x)."""
    import thinkdiff.ops  # noqa: F401
    ops = torch.ops.thinkdiff_hip
    D = 3072
    for rows in (4096, 8192):
        n_sets = 6
        sets = [[torch.randn(rows + 512, D, device="cuda").bfloat16()[512:] for _ in range(3)] for _ in range(n_sets)]
        st = {"i": 0}
        def head():
            st["i"] = (st["i"] + 1) % n_sets
            ops.block_cache_head(*sets[st["i"]])
        def tail():
            st["i"] = (st["i"] + 1) % n_sets
            ops.block_cache_tail(sets[st["i"]][0], sets[st["i"]][1])
        def copy_of(n_bufs):      # n_bufs x rows x D x 2 bytes moved: half read, half written
            elems = n_bufs * rows * D // 2
            src = [torch.randn(elems, device="cuda").bfloat16() for _ in range(n_sets)]
            dst = torch.empty(elems, device="cuda", dtype=torch.bfloat16)
            def f():
                st["i"] = (st["i"] + 1) % n_sets
                dst.copy_(src[st["i"]])
            return min(timeit(f, iters=50, warmup=5) for _ in range(3))
        t_head = min(timeit(head, iters=50, warmup=5) for _ in range(3))
        t_tail = min(timeit(tail, iters=50, warmup=5) for _ in range(3))
        c_head, c_tail = copy_of(4), copy_of(3)
        bh, bt = 4 * rows * D * 2, 3 * rows * D * 2
        print(f"block cache rows={rows} D={D}: head {t_head*1e3:.1f} us ({bh/1e6:.0f} MB, {bh/t_head/1e9:.2f} TB/s) vs copy of the same bytes {c_head*1e3:.1f} us "
              f"= {t_head/c_head:.2f}x;  tail {t_tail*1e3:.1f} us ({bt/1e6:.0f} MB, {bt/t_tail/1e9:.2f} TB/s) vs copy {c_tail*1e3:.1f} us = {t_tail/c_tail:.2f}x", flush=True)


def bench_gemmref():
    """External yardstick for the block GEMMs (measurement only; never in the product): torch.nn.functional.linear (= hipBLASLt on
    this image) against td_linear on the six FLUX.1-dev block shapes at the joint sequence length, random operands, same box, same
    process.  Two regimes: (a) per shape, cold weights (a 1.2 GB pool is cycled, as in the denoise loop where every layer has its
    own weights), interleaved rounds, best-of; (b) SUSTAINED: the six shapes back to back for ~3 s per backend, alternating
    backends -- the chip is power-limited on real data, so a short best-of flatters whichever kernel runs on a cool chip."""
    shapes = [("qkv", 4289, 9216, 3072), ("attn_out", 4289, 3072, 3072), ("ff1", 4289, 12288, 3072), ("ff2", 4289, 3072, 12288),
              ("single_in", 4289, 21504, 3072), ("single_out", 4289, 3072, 15360)]
    F = torch.nn.functional
    ops = {}
    for name, M, N, K in shapes:
        x = torch.randn(M, K, device="cuda").bfloat16()
        pool = [(torch.randn(N, K, device="cuda") * 0.02).bfloat16() for _ in range(max(2, int(1.2e9 // (N * K * 2))))]
        b = torch.randn(N, device="cuda").bfloat16()
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        st = {"i": 0}
        def ours(x=x, pool=pool, b=b, y=y, st=st):
            st["i"] = (st["i"] + 1) % len(pool)
            _hip.linear(x, pool[st["i"]], b, out=y)
        def lib(x=x, pool=pool, b=b, y=y, st=st):
            st["i"] = (st["i"] + 1) % len(pool)
            torch.addmm(b, x, pool[st["i"]].t(), out=y)
        ops[name] = (ours, lib, 2.0 * M * N * K)
        best = {"ours": 1e9, "lib": 1e9}
        for _ in range(4):
            best["ours"] = min(best["ours"], timeit(ours, iters=16, warmup=2))
            best["lib"] = min(best["lib"], timeit(lib, iters=16, warmup=2))
        fl = 2.0 * M * N * K
        print(f"{name:10s} M={M} N={N:5d} K={K:5d}: td_linear {best['ours']*1e3:7.1f} us {fl/best['ours']/1e9:6.0f} TF/s | "
              f"torch/hipBLASLt {best['lib']*1e3:7.1f} us {fl/best['lib']/1e9:6.0f} TF/s | ratio {best['lib']/best['ours']:.3f}", flush=True)
    # (b) sustained mix, weighted as one FLUX step: 19 x (qkv, attn_out, ff1, ff2) + 38 x (single_in, single_out)
    seq = [("qkv", 1), ("attn_out", 1), ("ff1", 1), ("ff2", 1), ("single_in", 2), ("single_out", 2)]
    fl_seq = sum(ops[n][2] * k for n, k in seq)
    def run_seq(which):
        for n, k in seq:
            for _ in range(k):
                ops[n][which]()
    res = {0: [], 1: []}
    for rnd in range(3):
        for which in (0, 1):
            run_seq(which); torch.cuda.synchronize()
            t0 = time.perf_counter(); n_it = 0
            while time.perf_counter() - t0 < 3.0:
                for _ in range(10):
                    run_seq(which)
                torch.cuda.synchronize(); n_it += 10
            el = time.perf_counter() - t0
            res[which].append(fl_seq * n_it / el / 1e12)
    print("sustained FLUX-step GEMM mix (3 s windows, alternating): td_linear " + " ".join(f"{v:6.0f}" for v in res[0]) +
          " TF/s | torch/hipBLASLt " + " ".join(f"{v:6.0f}" for v in res[1]) + " TF/s", flush=True)


def bench_attnref():
    """External yardstick for the joint attention (measurement only): torch SDPA (flash / CK backend on this image) on FLUX's shape."""
    for S, H in [(4289, 24), (4354, 24)]:
        W = H * 128
        pool = [torch.randn(1, S, 3 * W, device="cuda").bfloat16() for _ in range(6)]
        out = torch.empty(1, S, W, device="cuda", dtype=torch.bfloat16)
        st = {"i": 0}
        def ours():
            st["i"] = (st["i"] + 1) % len(pool)
            q = pool[st["i"]]
            _hip.attention(q[:, :, :W], q[:, :, W:2 * W], q[:, :, 2 * W:], out, H, H)
        def lib():
            st["i"] = (st["i"] + 1) % len(pool)
            q = pool[st["i"]].view(1, S, 3, H, 128)
            torch.nn.functional.scaled_dot_product_attention(q[:, :, 0].transpose(1, 2), q[:, :, 1].transpose(1, 2), q[:, :, 2].transpose(1, 2))
        best = {"ours": 1e9, "lib": 1e9}
        try:
            for _ in range(4):
                best["ours"] = min(best["ours"], timeit(ours, iters=10, warmup=2))
                best["lib"] = min(best["lib"], timeit(lib, iters=10, warmup=2))
        except Exception as e:  # noqa: BLE001
            print("torch SDPA failed:", e)
        fl = 4.0 * S * S * H * 128
        print(f"attn S={S} H={H}: td_attention {best['ours']*1e3:6.1f} us {fl/best['ours']/1e9:6.0f} TF/s | torch SDPA {best['lib']*1e3:6.1f} us {fl/best['lib']/1e9:6.0f} TF/s", flush=True)


def bench_flux():
    """Full FLUX.1-dev shape, cfg 2: S_img=4096, T=193, per-step time."""
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel
    import time
    t0 = time.time()
    m = FluxTransformer2DModel(max_img_tokens=4096, max_txt_tokens=512, max_steps=32)
    m.init_random(seed=1)
    torch.cuda.synchronize()
    print(f"create+init {time.time()-t0:.1f}s, params {m.num_parameters()/1e9:.3f} B", flush=True)
    T = 193
    pe = torch.randn(T, 4096, device="cuda").bfloat16() * 0.1
    pool = torch.randn(768, device="cuda").bfloat16()
    ids = torch.zeros(64, 64, 3)
    ids[..., 1] += torch.arange(64)[:, None]
    ids[..., 2] += torch.arange(64)[None, :]
    m.set_condition(pe, pool, ids.reshape(-1, 3))
    import numpy as np, math
    n = 28
    s = np.linspace(1.0, 1.0 / n, n); mu = 1.15
    s = math.exp(mu) / (math.exp(mu) + (1.0 / s - 1.0))
    sig = list(s.astype(np.float32)) + [0.0]
    m.set_timesteps([float(x) * 1000 for x in sig[:-1]], 3500.0)
    lat = torch.randn(4096, 64, device="cuda").bfloat16()
    out = torch.empty_like(lat)
    ms = timeit(lambda: m.forward_step(lat, 3, out), iters=5, warmup=2)
    print(f"flux forward step: {ms:.2f} ms  -> {68.27/ms*1e3/1e3:.1f} TF/s... ({68.27e12/ms/1e9:.0f} TF/s)", flush=True)
    x = lat.clone()
    t1 = time.time(); m.denoise(x, sig); torch.cuda.synchronize(); t2 = time.time()
    print(f"28-step denoise: {t2-t1:.3f} s/image, finite={bool(torch.isfinite(x.float()).all())}, std={float(x.float().std()):.3f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["gemm"])
    a = ap.parse_args()
    for w in a.what:
        globals()["bench_" + w]()
