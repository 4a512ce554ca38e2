"""Cases, float64 references, derived per-element bounds and deliberately wrong convolutions for the VAE's implicit-GEMM 3x3 convolutions
(csrc/gemm_bf16.hip gemm_tile, CONV = 1: stride 1 with an optional fused nearest 2x upsample; CONV = 2: stride 2 behind F.pad(x, (0, 1, 0, 1))),
shared by tests/test_vae_conv_cases_cpu.py and tests/test_vae_conv_fp64_gpu.py.  CPU only: nothing here touches a GPU.

Layouts are the kernel's: x [Hin, Win, Cin] bf16 (NHWC; the kernel takes it as [Hin * Win, Cin]), w [Cout, Cin, 3, 3] bf16 (torch's OIHW;
`pack` gives the kernel's [Cout, 9 Cin] with k = tap * Cin + c, tap = ky * 3 + kx), bias [Cout], res / output [M, Cout] with
M = Hout * Wout output pixels.  A case is
(form, H, W, Cin, Cout, res): H, W are the OUTPUT extent for `s1` and `up` (the input of `up` is H/2 x W/2) and the INPUT extent for `s2`
(its output is H/2 x W/2).

Rounding points (the tile epilogue of csrc/gemm_bf16.hip, `epilogue`): the fp32 accumulator plus the bias, in fp32, is the Linear output; without a
residual the final pack rounds it to bf16 once.  With a residual (mode 2) `round_all` rounds it to bf16 first, the residual is added in fp32, and
the final pack rounds the sum.  `expected` restates that chain in float64, `tol` bounds it:

    |y - inner| <= ulp_bf16(inner) + K 2^-24 absdot                      inner = dot + bias,   absdot = sum_k |x_k| |w_k|
    |y - ref|   <= the same + ulp_bf16(ref)                              ref = bf16(inner) + res, when there is a residual

the `linear_tol` / `sum_bound` reasoning of tests/qwen2_w8_common.py: the products of two bf16 values are exact in fp32, an fp32 sum of K of them
in ANY order is off by at most K 2^-24 absdot, and each rounding point costs one bf16 ulp of the value rounded (half an ulp for the rounding,
the rest for a value that the fp32 error pushed across a rounding boundary or into the next binade).  Through the residual sum the first point's error passes unchanged.  No bound comes from what a kernel returned.

Three operand makers, each seeded from the case: `integer` (values whose every partial sum is exact: the kernel must return bf16(ref) bit for bit),
`one_hot` (72 output channels that each copy one tap of one input channel: the expected output is written down by indexing, without a convolution)
and `random`.  `WRONG` holds convolutions that are wrong in the ways this kernel's addressing can be wrong; tests/test_vae_conv_cases_cpu.py shows
that every comparison rejects them, so that a kernel with one of these faults cannot pass tests/test_vae_conv_fp64_gpu.py.
"""
import functools
import json
import os

import torch
import torch.nn.functional as F

from qwen2_w8_common import sum_bound, ulp_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "vae_conv_fp64_bounds.json")

FORMS = ("s1", "up", "s2")
COUT_HOT = 72          # the one-hot maker's output channels: the 128-wide tile with a ragged n

# (form, H, W, Cin, Cout, res); which instantiation of launch_cfg<8, WN, CONV> td_gemm_launch routes a case to is `instantiation(case)`
CASES = [
    ("s1", 1, 7, 64, 8, False),          # a single row: no vertical tap is inside the image
    ("s1", 7, 1, 64, 64, False),         # a single column
    ("s1", 3, 3, 64, 64, False),         # every pixel is a border pixel
    ("s1", 16, 16, 128, 128, False),     # M = 256, exactly one m-tile
    ("s1", 1, 257, 64, 64, False),       # the second m-tile holds one row (255 rows past M)
    ("s1", 5, 260, 64, 32, False),       # an image row longer than an m-tile; Cout 32
    ("s1", 17, 31, 256, 256, True),      # odd width, tile rows straddle image rows, ragged last tile
    ("s1", 12, 20, 128, 192, False),     # ragged n in the 256-wide tile
    ("s1", 9, 33, 512, 512, True),       # K = 4608, two n-tiles
    ("s1", 4, 5, 192, 64, False),        # Cin / 64 = 3: the k-tile -> (tap, channel run) division by something that is no power of two
    ("up", 2, 2, 64, 64, False),         # 1x1 input
    ("up", 6, 10, 64, 128, False),       # 3x5 input
    ("up", 18, 30, 256, 256, True),      # 9x15 input (odd)
    ("up", 34, 16, 512, 512, False),     # M = 544, two n-tiles
    ("s2", 2, 2, 64, 64, False),         # one output pixel, 4 of 9 taps valid
    ("s2", 2, 10, 64, 8, False),         # one output row
    ("s2", 10, 2, 64, 32, False),        # one output column
    ("s2", 18, 30, 128, 128, False),     # 9x15 output
    ("s2", 34, 30, 256, 256, False),     # M = 255
    ("s2", 46, 24, 512, 512, False),     # M = 276, K = 4608, two n-tiles
]


def case_id(case):
    form, H, W, Cin, Cout, res = case
    return f"{form}-{H}x{W}-{Cin}to{Cout}" + ("-res" if res else "")


def extents(form, H, W):
    """(Hin, Win, Hout, Wout) of a case."""
    if form == "s1":
        return H, W, H, W
    if form == "up":
        assert H % 2 == 0 and W % 2 == 0
        return H // 2, W // 2, H, W
    assert form == "s2" and H % 2 == 0 and W % 2 == 0
    return H, W, H // 2, W // 2


def instantiation(case):
    """The kernel form td_gemm_launch (csrc/gemm_bf16.hip) routes the case to: N <= 64 the 64-wide output tile, N <= 128 the 128-wide, else the
    256-wide one; the stride-2 form is CONV = 2, the two others CONV = 1 (`true`)."""
    form, _, _, _, Cout, _ = case
    wn = 1 if Cout <= 64 else 2 if Cout <= 128 else 4
    return f"launch_cfg<8, {wn}, {'2' if form == 's2' else 'true'}>"


def _seed(case, maker):
    form, H, W, Cin, Cout, res = case
    return ((FORMS.index(form) * 1009 + H) * 1009 + W) * 4099 + Cin * 7 + Cout * 3 + maker * 1000003


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------

def to_nchw(x):
    """[Hin, Win, C] -> [1, C, Hin, Win]"""
    return x.permute(2, 0, 1)[None]


def out_extent(form, x):
    """The case's (H, W) from its input x [Hin, Win, Cin]: the output extent for s1 and up, the input extent for s2."""
    return (2 * x.shape[0], 2 * x.shape[1]) if form == "up" else (x.shape[0], x.shape[1])


def to_nhwc(t):
    """[1, C, H, W] -> [H * W, C]"""
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()


def pack(w, Cout_pad=None, Cin_pad=None):
    """torch's [Cout, Cin, 3, 3] -> the kernel's [Cout_pad, 9 Cin_pad], k = (ky * 3 + kx) * Cin_pad + c, zero filled: a permute and a pad
    (what td_conv3x3_pack_weight must give bit for bit)."""
    Cout, Cin = w.shape[:2]
    Cout_pad, Cin_pad = Cout_pad or Cout, Cin_pad or Cin
    out = torch.zeros(Cout_pad, 9, Cin_pad, dtype=w.dtype)
    out[:Cout, :, :Cin] = w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)
    return out.reshape(Cout_pad, 9 * Cin_pad)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def _conv64(form, x, w):
    xi = to_nchw(x)
    if form == "s1":
        y = F.conv2d(xi, w, padding=1)
    elif form == "up":
        y = F.conv2d(F.interpolate(xi, scale_factor=2, mode="nearest"), w, padding=1)
    else:
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), w, stride=2)
    return to_nhwc(y)


def ref(form, x, w, bias=None):
    """float64 F.conv2d on the CPU -> (dot, absdot), both [M, Cout] float64: the convolution alone, and the same convolution of |x| and |w|,
    the sum of magnitudes that the fp32 sum's error scales with.  The bias is not added here: it joins dot in `expected` and `tol`, where the
    rounding points are stated (the argument keeps one signature for this and the functions of WRONG)."""
    xd, wd = x.double(), w.double()
    return _conv64(form, xd, wd), _conv64(form, xd.abs(), wd.abs())


def bf(t):
    """One bf16 rounding of a float64 tensor."""
    return t.bfloat16().double()


def expected(dot, bias, res):
    """The kernel's rounding chain in float64 -> (what to compare with before the last rounding, the rounded value)."""
    inner = dot if bias is None else dot + bias.double()
    if res is None:
        return inner, bf(inner)
    r = bf(inner) + res.double()
    return r, bf(r)


def tol(dot, absdot, bias, res, K):
    """Per-element bound on |y - expected(...)[0]| (module docstring)."""
    inner = dot if bias is None else dot + bias.double()
    t = ulp_bf16(inner) + sum_bound(K, absdot)
    if res is not None:
        t = t + ulp_bf16(bf(inner) + res.double())
    return t


# ---- the geometry by indexing: a second statement of it, and the wrong ones -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tap_index(form, H, W, wrong=None):
    """idx [M, 9] int64: the flat input pixel that tap t = ky * 3 + kx of output pixel m reads, -1 where it reads the zero padding.  Plain loops
    over pixels and taps, no convolution.  wrong: one of the geometry faults of WRONG.  (Cached: the result is shared, not to be modified.)"""
    Hin, Win, Ho, Wo = extents(form, H, W)
    idx = torch.full((Ho * Wo, 9), -1, dtype=torch.int64)
    for y in range(Ho):
        for x in range(Wo):
            for t in range(9):
                ky, kx = divmod(t, 3)
                if form == "s2":
                    yy, xx = 2 * y + ky, 2 * x + kx
                    if wrong == "pad_top_left":
                        yy, xx = yy - 1, xx - 1
                    ok = 0 <= yy < Hin and 0 <= xx < Win
                    sy, sx = yy, xx
                    cy, cx = min(max(yy, 0), Hin - 1), min(max(xx, 0), Win - 1)
                else:
                    yy, xx = y + ky - 1, x + kx - 1
                    ok = 0 <= yy < Ho and 0 <= xx < Wo
                    up = 1 if form == "up" else 0
                    sy, sx = yy >> up, xx >> up
                    cy, cx = min(max(yy, 0), Ho - 1) >> up, min(max(xx, 0), Wo - 1) >> up
                    if wrong == "parent_before_tap":
                        sy, sx = (y >> 1) + ky - 1, (x >> 1) + kx - 1
                        ok = 0 <= sy < Hin and 0 <= sx < Win
                if wrong == "wrap":          # no validity test: the flat offset lands on the neighbouring row, or outside the buffer (zero)
                    flat = sy * Win + sx
                    src = flat if 0 <= flat < Hin * Win else -1
                elif wrong == "clamp":
                    src = cy * Win + cx
                else:
                    src = sy * Win + sx if ok else -1
                idx[y * Wo + x, t] = src
    if wrong == "rows_past_m":
        idx[-1] = idx[0]
    return idx


def _im2col(x, idx):
    """x [Hin, Win, Cin], idx [M, 9] -> A [M, 9, Cin] (zeros where idx is -1)"""
    x = x.reshape(-1, x.shape[-1])
    xz = torch.cat([x, torch.zeros(1, x.shape[1], dtype=x.dtype)])
    return xz[torch.where(idx < 0, x.shape[0], idx)]


def _wrong(name):
    def conv(form, x, w, bias=None):
        """`ref`'s signature; a float64 im2col product with one fault -> (dot, None)."""
        Cout, Cin = w.shape[:2]
        H, W = out_extent(form, x)
        geometry = name if name in ("wrap", "clamp", "pad_top_left", "parent_before_tap", "rows_past_m") else None
        A = _im2col(x.double(), tap_index(form, H, W, geometry))
        wp = pack(w.double())
        if name == "drop_last_chunk":
            A = A.clone()
            A[:, 8, Cin - 64:] = 0
        if name == "k_order":
            wp = w.double().reshape(Cout, Cin * 9)          # torch's own order, c * 9 + tap, read as if it were packed
        return A.reshape(A.shape[0], 9 * Cin) @ wp.t(), None
    conv.__name__ = name
    return conv


# wrap: border taps read the flat-index neighbour (no zero pad across row ends).  clamp: border taps read the clamped edge pixel.
# pad_top_left: the stride-2 form pads (1, 0, 1, 0) instead of (0, 1, 0, 1).  parent_before_tap: the upsampled form takes (y >> 1) + dy instead
# of (y + dy) >> 1.  drop_last_chunk: the last 64 input channels of tap 8 are missing.  k_order: weights read as c * 9 + tap.  rows_past_m: the
# last m-tile's missing rows alias pixel 0, so the last pixel's value is taken from pixel 0's taps.
WRONG = {name: _wrong(name) for name in ("wrap", "clamp", "pad_top_left", "parent_before_tap", "drop_last_chunk", "k_order", "rows_past_m")}
WRONG_FORMS = {"wrap": FORMS, "clamp": FORMS, "pad_top_left": ("s2",), "parent_before_tap": ("up",), "drop_last_chunk": FORMS, "k_order": FORMS,
               "rows_past_m": FORMS}


def applies(name, form, H, W):
    """Whether the fault changes what is read on this geometry at all.  It does not where its index map IS the right one: `wrap` on a one-row
    s1 image (every flat neighbour lies outside the buffer, which reads as zero), `rows_past_m` on a one-pixel output or one whose last pixel has
    pixel 0's taps, `drop_last_chunk` where tap 8 (dy = dx = +1) is inside the image for no pixel."""
    if form not in WRONG_FORMS[name]:
        return False
    right = tap_index(form, H, W)
    if name == "drop_last_chunk":
        return bool((right[:, 8] >= 0).any())
    if name == "k_order":
        return True
    return not torch.equal(tap_index(form, H, W, name), right)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------

def _gen(case, maker):
    return torch.Generator().manual_seed(_seed(case, maker))


def make_integer(case):
    """x, w in {-1, 0, 1} (non-zero with probability 1/2), bias integers in [-4, 4], res integers in [-8, 8].  While every |dot + bias| and
    |dot + bias + res| stays <= 256 (asserted on the float64 reference by whoever uses these), every partial sum in any order, the bias add and
    both bf16 roundings are exact, and the kernel must return the reference bit for bit."""
    form, H, W, Cin, Cout, res = case
    Hin, Win, Ho, Wo = extents(form, H, W)
    g = _gen(case, 0)
    tri = lambda *s: (torch.randint(0, 2, s, generator=g) * (2 * torch.randint(0, 2, s, generator=g) - 1)).bfloat16()
    x, w = tri(Hin, Win, Cin), tri(Cout, Cin, 3, 3)
    bias = torch.randint(-4, 5, (Cout,), generator=g).bfloat16()
    r = torch.randint(-8, 9, (Ho * Wo, Cout), generator=g).bfloat16() if res else None
    return x, w, bias, r


def make_random(case):
    """x randn, w randn / sqrt(9 Cin), bias and res randn, all bf16."""
    form, H, W, Cin, Cout, res = case
    Hin, Win, Ho, Wo = extents(form, H, W)
    g = _gen(case, 1)
    x = torch.randn(Hin, Win, Cin, generator=g).bfloat16()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).bfloat16()
    bias = torch.randn(Cout, generator=g).bfloat16()
    r = torch.randn(Ho * Wo, Cout, generator=g).bfloat16() if res else None
    return x, w, bias, r


def hot_weight(Cin, Cout_hot=COUT_HOT):
    """Output channel o has a single weight 1.0: tap o % 9, input channel (o // 9) * (Cin // 8) + 3."""
    w = torch.zeros(Cout_hot, Cin, 3, 3)
    for o in range(Cout_hot):
        w[o, (o // 9) * (Cin // 8) + 3, (o % 9) // 3, (o % 9) % 3] = 1.0
    return w.bfloat16()


def make_one_hot(case, Cout_hot=COUT_HOT):
    """x random finite non-zero bf16 values over 13 binades, the one-hot weight, no bias, no residual."""
    form, H, W, Cin, _, _ = case
    Hin, Win, _, _ = extents(form, H, W)
    g = _gen(case, 2)
    x = (torch.randn(Hin, Win, Cin, generator=g) * torch.exp2(torch.randint(-6, 7, (Hin, Win, Cin), generator=g).float())).bfloat16()
    assert bool(torch.isfinite(x).all()) and bool((x != 0).all())
    return x, hot_weight(Cin, Cout_hot)


def hot_expected(form, x, Cout_hot=COUT_HOT, wrong=None):
    """What the one-hot weight must give, by indexing alone: out[m, o] = x[pixel that tap o % 9 of m reads, channel of o], 0 outside the image."""
    Cin = x.shape[-1]
    idx = tap_index(form, *out_extent(form, x), wrong)
    x = x.reshape(-1, Cin)
    xz = torch.cat([x.double(), torch.zeros(1, Cin, dtype=torch.float64)])
    out = torch.empty(idx.shape[0], Cout_hot, dtype=torch.float64)
    for o in range(Cout_hot):
        src = idx[:, o % 9]
        out[:, o] = xz[torch.where(src < 0, x.shape[0], src), (o // 9) * (Cin // 8) + 3]
    return out


@functools.lru_cache(maxsize=None)
def reference(case, maker):
    """The operands of (case, maker) and what they must give, computed once per process and shared; nothing in it is to be modified.
    maker: "integer" or "random".  -> dict(x, w, bias, res, dot, absdot, cmp, want, tol)"""
    form, H, W, Cin, Cout, _ = case
    x, w, bias, r = (make_integer if maker == "integer" else make_random)(case)
    dot, absdot = ref(form, x, w, bias)
    cmp, want = expected(dot, bias, r)
    return dict(x=x, w=w, bias=bias, res=r, dot=dot, absdot=absdot, cmp=cmp, want=want, tol=tol(dot, absdot, bias, r, 9 * Cin))


def integer_condition(dot, bias, res):
    """The largest magnitude any exact partial result of the integer maker can be asked to hold; the maker's claim needs it <= 256."""
    inner = dot + bias.double()
    m = float(inner.abs().max())
    return m if res is None else max(m, float((inner + res.double()).abs().max()))


# ---- comparisons (a got tensor is float64 [M, Cout]) ------------------------------------------------------------------------------------

def check_exact(got, want, what):
    """Every element equal as a value (+0.0 == -0.0), all finite."""
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), what
    bad = got != want
    if bool(bad.any()):
        i = int(torch.argmax(bad.reshape(-1).int()))
        m, o = divmod(i, want.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements differ; first at pixel {m} channel {o}: got {float(got[m, o])!r} "
                             f"want {float(want[m, o])!r}")


def check_tol(got, cmp, t, what):
    """Every element within its bound; prints and returns the worst error / bound ratio."""
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), what
    ratio = (got - cmp).abs() / t
    worst = float(ratio.max())
    print(f"{what}: max error {worst:.3f} x the bound")
    if worst > 1.0:
        i = int(torch.argmax(ratio))
        m, o = divmod(i, cmp.shape[1])
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} / {ratio.numel()} elements beyond the bound; worst at pixel {m} channel {o}: got "
                             f"{float(got[m, o]):.6g} ref {float(cmp[m, o]):.6g} ({worst:.3g} x the bound)")
    return worst


def record(key, ratio):
    """Keep the worst error / bound ratio of one case in profiles/vae_conv_fp64_bounds.json (a record; no bound is read from it)."""
    print(f"{key}: worst error / bound = {ratio:.4f}")
    try:
        with open(RECORD) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    data[key] = round(float(ratio), 4)
    try:
        with open(RECORD, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:      # a read-only checkout still runs the assertions
        pass
