"""What the tile GEMM launches write, as digests: the record behind a refactor of csrc/gemm_bf16.hip (profiles/gemm_one_tile_body.md).  The GPU
tests compare one launch form of a build with another form of the same build; this compares two BUILDS: run it from each build's tree.

--out FILE.json   runs a fixed list of launches through thinkdiff._hip (the C ABI of this tree's library; no torch.ops) on seeded inputs and writes one
                  sha256 per launch over its whole output buffers -- guard rows behind M and pad columns behind N included, as
                  tests/test_gemm_drain_gpu.py builds them.  Shapes are the smallest at which each path can still go wrong (ragged row and column
                  tiles, one-row tiles, k-loops shorter than the walk drains under, several tiles per workgroup): the persistent walk
                  (linear_drain), the one-tile launch on the 256x256 and the 288x192 tile, both under TD_GEMM_DRAIN unset / 0 / 1, the tail
                  split (TD_GEMM_TAIL=2 / 4), the int8 and e4m3 kernels, the int8-output form, the K split and the 3x3 convolutions.
--compare A B     lists the entries in which two such files differ; exit status 1 if there are any.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thinkdiff-mlre_amd"))
from thinkdiff import _hip as hip  # noqa: E402

PAD = 8      # columns behind N in every output row, three guard rows behind M: a launch must not touch them


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:24]


def rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).bfloat16().cuda()


def out(M, N, fill=0.5):
    buf = torch.full((M + 3, N + PAD), fill, dtype=torch.bfloat16, device="cuda")
    return buf, buf[:M, :N]


class Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def walk_cases():
    """(name, fn -> output buffers) through td_linear_drain_bf16: tests/test_gemm_drain_gpu.py's problems."""
    cases = []
    for K in (128, 64):      # 513 rows: the last row tile holds one row (ragged loop); two k-tiles and one: fewer than the walk drains under
        g = torch.Generator().manual_seed(K)
        x, w, b = rand(g, 513, K), rand(g, 512, K, scale=0.05), rand(g, 512)

        def f(x=x, w=w, b=b):
            buf, y = out(513, 512)
            hip.linear_drain(x, w, b, y, max_workgroups=1)
            return [buf]
        cases.append((f"walk_513x512x{K}_wg1", f))
    g = torch.Generator().manual_seed(11)
    M, N, K = 600, 768, 3072
    x, w, b, gate, h0 = rand(g, M, K), rand(g, N, K, scale=0.02), rand(g, N), rand(g, N), rand(g, M + 3, N + PAD)

    def f_bias():
        buf, y = out(M, N)
        hip.linear_drain(x, w, b, y, max_workgroups=2)
        return [buf]

    def f_gated():
        buf = h0.clone()
        y = buf[:M, :N]
        hip.linear_drain(x, w, b, y, gate0=gate, res0=y, max_workgroups=2)
        return [buf]
    cases += [("walk_600x768x3072_wg2_bias", f_bias), ("walk_600x768x3072_wg2_gated_residual_in_place", f_gated)]
    g = torch.Generator().manual_seed(12)
    M0, M1, Ng, Kg = 300, 70, 512, 256
    p0 = (rand(g, M0, Kg), rand(g, Ng, Kg, scale=0.05), rand(g, Ng), rand(g, Ng), rand(g, M0, Ng + PAD))
    p1 = (rand(g, M1, Kg), rand(g, Ng, Kg, scale=0.05), rand(g, Ng), rand(g, Ng), rand(g, M1, Ng + PAD))

    def f_grouped():
        buf0, y0 = out(M0, Ng)
        buf1, y1 = out(M1, Ng)
        hip.linear_drain(p0[0], p0[1], p0[2], y0, p1[0], p1[1], p1[2], y1, gate0=p0[3], res0=p0[4][:, :Ng], gate1=p1[3], res1=p1[4][:, :Ng], max_workgroups=2)
        return [buf0, buf1]
    cases.append(("walk_grouped_300+70x512x256_wg2", f_grouped))
    g = torch.Generator().manual_seed(13)
    xs, ws, bs = rand(g, 300, 256), rand(g, 768, 256, scale=0.05), rand(g, 768)

    def f_split():
        buf0, y0 = out(300, 256)
        buf1, y1 = out(300, 512)
        hip.linear_drain(xs, ws, bs, y0, y_split=y1, act_split=hip.ACT_GELU_TANH, n_split=256, max_workgroups=1)
        return [buf0, buf1]
    cases.append(("walk_split_300x768x256_gelu_second", f_split))
    g = torch.Generator().manual_seed(14)
    xr, wr, br, rr = rand(g, 257, 256), rand(g, 328, 256, scale=0.05), rand(g, 328), rand(g, 257, 328 + PAD)

    def f_res():
        buf, y = out(257, 328)
        hip.linear_drain(xr, wr, br, y, res0=rr[:, :328], max_workgroups=1)
        return [buf]
    cases.append(("walk_257x328x256_residual", f_res))
    return cases


def one_tile_cases():
    """(name, fn) through td_linear_grouped2_bf16 on the 256x256 (tile_cfg 0) and the 288x192 (3) tile: tests/test_gemm_tile_identity_gpu.py's
    problems, and 258 / 4354 rows: whole 256-row tiles plus two rows (the ragged loop of the 256x256 tile)."""
    cases = []
    shapes = [(300, 0, 392, 192, ("bias", "gelu", "gated")), (577, 0, 200, 128, ("bias", "gelu", "gated")), (260, 70, 392, 192, ("bias", "gated")),
              (258, 0, 768, 512, ("bias",)), (4354, 0, 768, 384, ("gated",))]
    for M, M1, N, K, forms in shapes:
        g = torch.Generator().manual_seed(M + N)
        p0 = (rand(g, M, K), rand(g, N, K, scale=0.05), rand(g, N), rand(g, N), rand(g, M + 3, N + PAD))
        p1 = (rand(g, M1, K), rand(g, N, K, scale=0.05), rand(g, N), rand(g, N), rand(g, M1 + 3, N + PAD)) if M1 else None
        for cfg in (0, 3):
            for form in forms:
                def f(p0=p0, p1=p1, M=M, M1=M1, N=N, cfg=cfg, form=form):
                    buf0 = p0[4].clone()
                    y0 = buf0[:M, :N]
                    x1 = w1 = b1 = g1 = y1 = buf1 = None
                    if p1 is not None:
                        buf1 = p1[4].clone()
                        x1, w1, b1, g1, y1 = p1[0], p1[1], p1[2], p1[3], buf1[:M1, :N]
                    if form == "gated":      # y += gate * (x W^T + b), in place
                        hip.linear_grouped2(p0[0], p0[1], p0[2], y0, x1, w1, b1, y1, gate0=p0[3], res0=y0, gate1=g1, res1=y1, tile_cfg=cfg)
                    else:
                        hip.linear_grouped2(p0[0], p0[1], p0[2], y0, x1, w1, b1, y1, act=hip.ACT_GELU_TANH if form == "gelu" else hip.ACT_NONE, tile_cfg=cfg)
                    return [buf0] + ([buf1] if buf1 is not None else [])
                cases.append((f"tile{cfg}_{M}+{M1}x{N}x{K}_{form}", f))
    return cases


def tail_case():
    """4096 + 193 rows x 12288 x 256: 816 tiles of 256x256, more than three rounds of the CUs -- the launch the tail split cuts."""
    g = torch.Generator().manual_seed(21)
    M0, M1, N, K = 4096, 193, 12288, 256
    x0, x1, w0, w1, b = rand(g, M0, K), rand(g, M1, K), rand(g, N, K, scale=0.05), rand(g, N, K, scale=0.05), rand(g, N)

    def f():
        buf0, y0 = out(M0, N)
        buf1, y1 = out(M1, N)
        hip.linear_grouped2(x0, w0, b, y0, x1, w1, b, y1, act=hip.ACT_GELU_TANH, tile_cfg=0)
        return [buf0, buf1]
    return f


def eight_bit_cases():
    cases = []
    g = torch.Generator().manual_seed(31)
    M, N, K = 300, 512, 256
    x, w, b, gate, r = rand(g, M, K), rand(g, N, K, scale=0.05), rand(g, N), rand(g, N), rand(g, M, N + PAD)
    for kind, quant, lin in (("int8", hip.quant_rows_int8, hip.linear_int8), ("fp8", hip.quant_rows_fp8, hip.linear_fp8)):
        xq, xs = quant(x)
        wq, ws = quant(w)
        for cfg in (0, 2, 3):
            def f(lin=lin, xq=xq, xs=xs, wq=wq, ws=ws, cfg=cfg):
                buf0, y0 = out(M, N)
                buf1, y1 = out(M, N)
                lin(xq, xs, wq, ws, b, act=hip.ACT_GELU_TANH, out=y0, tile_cfg=cfg)
                lin(xq, xs, wq, ws, b, gate=gate, res=r[:, :N], out=y1, tile_cfg=cfg)
                return [buf0, buf1]
            cases.append((f"linear_{kind}_300x512x256_tile{cfg}", f))
    xq, xs = hip.quant_rows_int8(x)
    wq, ws = hip.quant_rows_int8(w)
    inv = (torch.rand(M, generator=g) * 20.0 + 5.0).cuda()
    smooth = torch.exp2(torch.randint(-2, 3, (N,), generator=g).float()).bfloat16().cuda()
    for cfg in (0, 2):
        for sm in (None, smooth):
            def f(cfg=cfg, sm=sm):
                ldq8 = N + 48
                buf = torch.full((M + 3, ldq8), 77, dtype=torch.int8, device="cuda")
                amax = torch.zeros(M + 2, dtype=torch.int32, device="cuda")
                pr = hip.q8_problem(xq, xs, wq, ws, b, buf, inv, amax, sm)
                hip.linear_int8_q8(pr, N, K, ldx=K, ldq8=ldq8, act=hip.ACT_GELU_TANH, tile_cfg=cfg)
                return [buf, amax]
            cases.append((f"linear_int8_q8_300x512x256_tile{cfg}_smooth{int(sm is not None)}", f))
    return cases


def splitk_and_conv_cases():
    cases = []
    g = torch.Generator().manual_seed(41)
    M, N, K = 130, 4096, 512
    x, w, b, r = rand(g, M, K), rand(g, N, K, scale=0.05), rand(g, N), rand(g, M, N + PAD)

    def f_sk():
        buf, y = out(M, N)
        hip.linear_splitk(x, w, b, res=r[:, :N], out=y, split_k=-1)
        return [buf]
    cases.append(("linear_splitk_130x4096x512", f_sk))
    H = W = 16
    for cin, cout in ((64, 64), (64, 128), (64, 256)):      # the 64-, 128- and 256-column conv tiles
        g = torch.Generator().manual_seed(cin + cout)
        xi = rand(g, H * W, cin)
        wt = hip.conv3x3_pack_weight(rand(g, cout, cin, 3, 3, scale=(9 * cin) ** -0.5))
        bc, rc = rand(g, cout), rand(g, H * W, cout)
        xh = rand(g, (H // 2) * (W // 2), cin)
        cases.append((f"conv3x3_16x16_{cin}to{cout}", lambda xi=xi, wt=wt, bc=bc, cout=cout: [hip.conv3x3_nhwc(xi, wt, bc, H, W, cout)]))
        cases.append((f"conv3x3_16x16_{cin}to{cout}_residual", lambda xi=xi, wt=wt, bc=bc, rc=rc, cout=cout: [hip.conv3x3_nhwc(xi, wt, bc, H, W, cout, res=rc)]))
        cases.append((f"conv3x3_up2x_to16x16_{cin}to{cout}", lambda xh=xh, wt=wt, bc=bc, cout=cout: [hip.conv3x3_nhwc(xh, wt, bc, H, W, cout, upsample2x=True)]))
        cases.append((f"conv3x3_s2_16x16_{cin}to{cout}", lambda xi=xi, wt=wt, bc=bc, cout=cout: [hip.conv3x3_s2_nhwc(xi, wt, bc, H, W, cout)]))
    return cases


def run_digests(path):
    res = {}

    def run(name, fn):
        bufs = fn()
        torch.cuda.synchronize()
        res[name] = sha(*bufs)

    tile_cases = walk_cases() + one_tile_cases()
    for drain in (None, "0", "1"):
        with Env(TD_GEMM_DRAIN=drain, TD_GEMM_TAIL=None):
            for name, fn in tile_cases:
                run(f"TD_GEMM_DRAIN={drain if drain is not None else 'unset'}/{name}", fn)
    tail = tail_case()
    for split in (None, "2", "4"):
        with Env(TD_GEMM_TAIL=split, TD_GEMM_DRAIN=None):
            run(f"TD_GEMM_TAIL={split if split is not None else 'unset'}/tile0_4096+193x12288x256_gelu", tail)
    with Env(TD_GEMM_TAIL=None, TD_GEMM_DRAIN=None):
        for name, fn in eight_bit_cases() + splitk_and_conv_cases():
            run(name, fn)
    with open(path, "w") as fh:      # (one line per launch)
        fh.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(res[k])}" for k in sorted(res)) + "\n}\n")
    print(f"wrote {len(res)} entries to {path}")


def compare(a, b):
    A, Bv = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(A) | set(Bv) if A.get(k) != Bv.get(k))
    for k in diff:
        print("differs:", k)
    print(f"{len(diff)} of {len(set(A) | set(Bv))} entries differ between {a} and {b}")
    return 1 if diff else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    assert torch.cuda.is_available(), "gemm_digest.py runs the kernels on the MI355X; there is no CPU path"
    if a.out:
        run_digests(a.out)


if __name__ == "__main__":
    main()
