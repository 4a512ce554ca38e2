"""The two pieces the VAE mid-block attention (mid_attention in csrc/vae_common.h) is built from, each against float64:
td_linear_f32out_bf16 (the GEMM's fp32-output epilogue, with the tile-config choice of its own that the entry and mid_attention share) and
td_softmax_rows_f32_bf16 / td_softmax_rows_strided_f32_bf16.  The whole-model VAE tests reach them only through a relative RMSE of 3e-2 over an
image, with at most 256 keys.

fp32-output Linear: y = x . w^T (+ bias) leaves the kernel unrounded, so the bound is the worst-case fp32 summation bound for ANY order of
the K products and the bias: |y - ref| <= (K + 2) 2^-24 (sum_k |x_ik w_jk| + |bias_j|), ref in float64 from the bf16 operands (products of two
bf16 values are exact in fp32).  With operands uniform in [0, 1) nothing cancels, the bound is ~ (K + 2) 2^-24 ~ 3e-5 relative at K = 512, and an
output that passed through bf16 on its way (2^-9 relative) misses it by two orders of magnitude.

Row softmax: the model of tests/test_epilogues_gpu.py.  The kernel works in fp32 (row maximum, exp2 of (s - max) * scale * log2 e, sum,
reciprocal) and rounds once to bf16, so every element lies within 1 bf16 ulp of bf16(float64 softmax), with an absolute floor of 2^-30, and it
differs from it at all only where the float64 value lies within a few fp32 ulps of a bf16 rounding boundary (expected rate: the fp32 error of an
element, <= ~4e-6 relative far below the maximum, over the bf16 spacing 2^-8: ~0.1 %).  At least 99 % of the elements at or above 2^-13 must be
bit-equal: a rate, so it is asserted over the pooled elements of every (cols, input kind) and for every single launch that has >= 200 such
elements (a launch with 30 of them would fail on one legitimate near-tie).

Measured on MI355X: fp32-output Linear at most 0.019 x the bound (randn and uniform operands, all three tile configs, strided rows); softmax
never beyond 1 bf16 ulp, pooled bit-equal rate >= 0.99994 for every (cols, input kind).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -7.0


def _linear_f32out(hip, x, w, bias, y, M, N, K):
    hip.check(hip.lib().td_linear_f32out_bf16(hip.ptr(x), x.stride(0), hip.ptr(w), hip.ptr(bias), hip.ptr(y), y.stride(0), M, N, K, hip.stream_ptr()))


def _operands(M, N, K, kind, seed):
    g = torch.Generator().manual_seed(seed)
    draw = (lambda *s: torch.rand(*s, generator=g)) if kind == "uniform" else (lambda *s: torch.randn(*s, generator=g))
    return draw(M, K).bfloat16(), draw(N, K).bfloat16(), draw(N).bfloat16()


def _check_linear(y, x, w, bias, what):
    """y fp32 [M, N] (cpu) against float64 with the summation bound of the module docstring; returns the worst ratio."""
    K = x.shape[1]
    ref = x.double() @ w.double().T
    mag = x.double().abs() @ w.double().abs().T
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    bound = (K + 2) * 2.0 ** -24 * mag
    assert torch.isfinite(y).all(), what
    ratio = ((y.double() - ref).abs() / bound.clamp_min(2.0 ** -140)).max().item()
    print(f"{what}: max error {ratio:.3f} x the bound; max |err| / max |ref| = {float((y.double() - ref).abs().max() / ref.abs().max()):.3e}")
    assert ratio <= 1.0, f"{what}: max error {ratio:.3f} x the bound"
    return ratio


# (M, N, K): the entry picks tile config 1 (64 columns) for N <= 64, else 2 (32 rows x 256 columns) for M <= 32, else 0 (256 x 256) -- both sides of
# each threshold, the smallest problem, N that is no multiple of a tile (72, 520), M past one 256-row tile (300); K a multiple of the 64-wide k-tile
LINEAR_SHAPES = [(1, 64, 64), (33, 64, 128), (32, 512, 64), (17, 72, 128), (33, 512, 128), (200, 128, 192), (300, 520, 320)]


@pytest.mark.parametrize("with_bias", [False, True], ids=["no_bias", "bias"])
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_linear_f32out_against_float64(hip, M, N, K, with_bias):
    x, w, b = _operands(M, N, K, "randn", M * 7 + N * 3 + K)
    bias = b if with_bias else None
    y = torch.full((M, N), SENT, dtype=torch.float32, device="cuda")
    _linear_f32out(hip, x.cuda(), w.cuda(), None if bias is None else bias.cuda(), y, M, N, K)
    torch.cuda.synchronize()
    _check_linear(y.cpu(), x, w, bias, f"fp32-output Linear M={M} N={N} K={K} bias={with_bias}")


@pytest.mark.parametrize("M,N,K", [(200, 128, 512), (32, 512, 512), (40, 64, 512)])
def test_linear_f32out_is_not_rounded_on_the_way(hip, M, N, K):
    """Operands uniform in [0, 1): the bound is ~3e-5 relative, a bf16 round trip (2^-9) fails it.  One shape per tile config."""
    x, w, b = _operands(M, N, K, "uniform", M + N + K)
    y = torch.full((M, N), SENT, dtype=torch.float32, device="cuda")
    _linear_f32out(hip, x.cuda(), w.cuda(), b.cuda(), y, M, N, K)
    torch.cuda.synchronize()
    yc = y.cpu()
    _check_linear(yc, x, w, b, f"fp32-output Linear, uniform operands, M={M} N={N} K={K}")
    ref = x.double() @ w.double().T + b.double()
    assert float(((ref.bfloat16().double() - ref).abs() / ((K + 2) * 2.0 ** -24 * ref.abs())).max()) > 10.0      # the input condition: rounding to bf16 would be seen


@pytest.mark.parametrize("M,N,K", [(33, 64, 128), (17, 72, 128), (300, 520, 320)])
def test_linear_f32out_strided_rows(hip, M, N, K):
    """ldx > K and ldy > N: the pad columns of y keep their sentinel and the rows past M are untouched."""
    x, w, b = _operands(M, N, K, "randn", M + 2 * N + 3 * K)
    xw = torch.full((M, K + 8), 1e4, dtype=torch.bfloat16)
    xw[:, :K] = x
    dx = xw.cuda()
    y = torch.full((M + 3, N + 8), SENT, dtype=torch.float32, device="cuda")
    _linear_f32out(hip, dx[:, :K], w.cuda(), b.cuda(), y, M, N, K)
    torch.cuda.synchronize()
    yc = y.cpu()
    _check_linear(yc[:M, :N], x, w, b, f"fp32-output Linear, strided rows, M={M} N={N} K={K}")
    assert (yc[:M, N:] == SENT).all(), "pad columns of y written"
    assert (yc[M:] == SENT).all(), "rows past M written"


# ---- row softmax -------------------------------------------------------------------------------------------------------------------------------------

FLOOR = 2.0 ** -30


def _ulp(r):
    a = r.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _softmax_inputs(rows, cols, g):
    """{kind: fp32 [rows, cols] on the device}: randn x 8; a +40 spike per row at column 0, cols - 1, 1023, 1024 (where they exist; the last
    two are the last element of the workgroup's first pass over the row and the first of its second); a common offset of +1e4; constant rows."""
    base = lambda: torch.randn(rows, cols, generator=g, device="cuda") * 8.0
    out = {"randn x 8": base()}
    for c in sorted({0, cols - 1, 1023, 1024}):
        if c < cols:
            s = base()
            s[:, c] += 40.0
            out[f"+40 at column {c}"] = s
    out["offset +1e4"] = base() + 1.0e4
    out["constant rows"] = (torch.arange(rows, device="cuda", dtype=torch.float32)[:, None] * 1.25 - 3.0).expand(rows, cols).contiguous()
    return out


@pytest.mark.parametrize("cols", [4, 60, 64, 1020, 1024, 1028, 4096, 16384])
def test_softmax_rows_against_float64(hip, cols):
    """rows 1, 3, 257 x scale 1, 512^-0.5 x (the unstrided entry with ld = cols, the strided entry with ld = the next multiple of 64 above cols).
    In the strided case the pad columns of s hold NaN (never read: a NaN would poison the row) and those of p come back as exact zeros;
    the row behind the last one keeps its sentinel.  Reference: float64 softmax(scale * s) of the fp32 scores, on the device."""
    L = hip.lib()
    g = torch.Generator(device="cuda").manual_seed(cols)
    pooled, worst = {}, 0.0
    for rows in (1, 3, 257):
        for kind, s in _softmax_inputs(rows, cols, g).items():
            for scale in (1.0, 512 ** -0.5):
                f_scale = ctypes.c_float(scale)
                ref64 = torch.softmax(s.double() * f_scale.value, dim=1)
                ref = ref64.bfloat16()
                for ld in (cols, (cols // 64 + 1) * 64):
                    p = torch.full((rows + 1, ld), SENT, dtype=torch.bfloat16, device="cuda")
                    if ld == cols:
                        hip.check(L.td_softmax_rows_f32_bf16(hip.ptr(s), hip.ptr(p), rows, cols, f_scale, hip.stream_ptr()))
                    else:
                        sp = torch.full((rows, ld), float("nan"), dtype=torch.float32, device="cuda")
                        sp[:, :cols] = s
                        hip.check(L.td_softmax_rows_strided_f32_bf16(hip.ptr(sp), hip.ptr(p), rows, cols, ld, f_scale, hip.stream_ptr()))
                    torch.cuda.synchronize()
                    what = f"softmax rows={rows} cols={cols} ld={ld} scale={scale:.4f} '{kind}'"
                    assert (p[rows].float() == SENT).all(), what + ": the row behind the last one was written"
                    assert (p[:rows, cols:].view(torch.int16) == 0).all(), what + ": pad columns of p are not exact zeros"
                    got = p[:rows, :cols]
                    gd, rd = got.double(), ref.double()
                    assert torch.isfinite(gd).all(), what
                    ratio = float(((gd - rd).abs() / torch.clamp_min(_ulp(rd), FLOOR)).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, what + f": max error {ratio:.3f} x (1 bf16 ulp, floor 2^-30)"
                    sel = rd >= 2.0 ** -13
                    n, same = int(sel.sum()), int((got.view(torch.int16) == ref.view(torch.int16))[sel].sum())
                    if n >= 200:
                        assert same >= 0.99 * n, what + f": only {same} of {n} elements >= 2^-13 bit-equal to the reference"
                    acc = pooled.setdefault(kind, [0, 0])
                    acc[0] += same
                    acc[1] += n
    for kind, (same, n) in pooled.items():      # (n = 0: constant rows of 16384 columns, every element 2^-14 -- the 1-ulp bound alone)
        print(f"softmax cols={cols} '{kind}': {same} of {n} elements >= 2^-13 bit-equal ({same / max(n, 1):.5f})")
        assert same >= 0.99 * n, f"softmax cols={cols} '{kind}': only {same} of {n} elements >= 2^-13 bit-equal to the reference"
    print(f"softmax cols={cols}: max error {worst:.3f} x (1 bf16 ulp, floor 2^-30)")
