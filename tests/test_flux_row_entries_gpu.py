"""The small kernels of the FLUX step, each launched alone: the temb combine + SiLU and the column copy (which had no entry point and so
no kernel test), the RoPE table, the timestep embedding and the counter-based normal fill.  References are float64 (or, where the result
is a chain of exactly rounded fp32 / bf16 operations, that chain on the CPU, bit for bit); bounds are derived next to each test and the
measured worst error / bound ratios go to profiles/flux_rowops_fp64_bounds.json.
"""
import ctypes
import math

import pytest
import torch

import flux_rowops_common as C

pytestmark = pytest.mark.gpu

SENTINEL = -3.0


# ---- td_temb_combine_silu_bf16 --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [8, 100, 3072])
@pytest.mark.parametrize("n", [1, 3])
def test_temb_combine_silu(hip, n, D):
    """temb = bf16(bf16(te + ge) + pe) bit for bit (two fp32 additions of bf16 values, each rounded to bf16: IEEE operations, the same
    on the CPU); silu_out within one bf16 ulp of float64 SiLU of that temb plus 4 * 2^-24 |value| (fp32 exp, reciprocal and product in
    front of the one rounding).  With and without ge, with and without the temb output; values at +-20 and 0 included."""
    g = torch.Generator().manual_seed(n * 10000 + D)
    te = (torch.randn(n, D, generator=g) * 3).bfloat16()
    ge = torch.randn(D, generator=g).bfloat16()
    pe = torch.randn(D, generator=g).bfloat16()
    te[0, :6] = torch.tensor([20.0, -20.0, 0.0, 1.0, -1.0, 0.0]).bfloat16()
    ge[:6] = torch.tensor([0.0, 0.0, 0.0, -1.0, 0.5, 20.0]).bfloat16()
    pe[:6] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.5, -40.0]).bfloat16()        # temb 20, -20, 0, 0, 0, -20
    worst = 0.0
    for use_ge in (True, False):
        t = te.float()
        if use_ge:
            t = (t + ge.float()).bfloat16().float()
        temb_ref = (t + pe.float()).bfloat16()
        v = temb_ref.double()
        silu_ref = C.bf(v / (1.0 + torch.exp(-v)))
        tol = C._ulp(silu_ref) + 4 * 2.0 ** -24 * silu_ref.abs()
        for want_temb in (True, False):
            temb, silu = hip.temb_combine_silu(te.cuda(), ge.cuda() if use_ge else None, pe.cuda(), want_temb=want_temb)
            torch.cuda.synchronize()
            what = f"temb_combine_silu n={n} D={D} ge={use_ge} temb={want_temb}"
            if want_temb:
                assert torch.equal(C.bits(temb), C.bits(temb_ref)), what + ": temb is not bf16(bf16(te + ge) + pe)"
            worst = max(worst, C._check(silu, silu_ref, tol, what))
    assert worst <= 1.0
    C.record(f"temb_combine_silu[n={n},D={D}]", worst)


def test_temb_combine_silu_refusals(hip):
    L = hip.lib()
    t = torch.zeros(8, dtype=torch.bfloat16, device="cuda")
    p = hip.ptr(t)
    for what, args in [("te null", (None, None, p, 1, 8, None, p, None)), ("pe null", (p, None, None, 1, 8, None, p, None)),
                       ("silu_out null", (p, None, p, 1, 8, p, None, None)), ("n = 0", (p, None, p, 0, 8, None, p, None)),
                       ("D = 0", (p, None, p, 1, 0, None, p, None))]:
        assert L.td_temb_combine_silu_bf16(*args) == 2, what
        assert b"td_temb_combine_silu" in L.td_last_error(), what


# ---- td_copy_cols_bf16 --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,lds,ldd", [(1, 8, 8, 16), (37, 64, 64, 128), (5, 320, 328, 384)])
def test_copy_cols_bit_exact(hip, rows, cols, lds, ldd):
    """dst[:, :cols] = src[:, :cols] bit for bit; the columns of dst behind cols keep their sentinel.  37 x 64 / 8 = 296 lanes: two blocks,
    the second partial."""
    g = torch.Generator().manual_seed(rows)
    src = torch.randn(rows, lds, generator=g).bfloat16()
    src.view(-1)[:3] = torch.tensor([-0.0, float("inf"), 1e-40]).bfloat16()       # bits, not values
    dst = torch.full((rows, ldd), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hip.copy_cols(src.cuda(), dst, cols)
    torch.cuda.synchronize()
    assert torch.equal(C.bits(dst)[:, :cols], C.bits(src)[:, :cols])
    assert (dst[:, cols:].cpu().float() == SENTINEL).all(), "columns of dst behind cols written"


def test_copy_cols_refusals(hip):
    """cols no multiple of 8, cols beyond ldd (or lds), a stride that is no multiple of 8 and a pointer that is not 16-byte aligned are
    refused before the launch: dst keeps its bits."""
    L = hip.lib()
    src = torch.zeros(4, 64, dtype=torch.bfloat16, device="cuda")
    dst = torch.full((4, 64), SENTINEL, dtype=torch.bfloat16, device="cuda")
    s, d, i64 = src.data_ptr(), dst.data_ptr(), ctypes.c_int64
    vp = ctypes.c_void_p
    for what, args in [("cols % 8", (vp(s), i64(64), vp(d), i64(64), 4, 12, None)), ("cols > ldd", (vp(s), i64(64), vp(d), i64(32), 4, 40, None)),
                       ("cols > lds", (vp(s), i64(32), vp(d), i64(64), 4, 40, None)), ("ldd % 8", (vp(s), i64(64), vp(d), i64(60), 4, 8, None)),
                       ("src misaligned", (vp(s + 8), i64(32), vp(d), i64(64), 4, 8, None)), ("dst misaligned", (vp(s), i64(64), vp(d + 8), i64(32), 4, 8, None)),
                       ("rows = 0", (vp(s), i64(64), vp(d), i64(64), 0, 8, None)), ("src null", (None, i64(64), vp(d), i64(64), 4, 8, None)),
                       ("ldd beyond 32 bits", (vp(s), i64(64), vp(d), i64(2 ** 31), 4, 8, None))]:
        assert L.td_copy_cols_bf16(*args) == 2, what
        assert b"td_copy_cols" in L.td_last_error(), what
    torch.cuda.synchronize()
    assert (dst.cpu().float() == SENTINEL).all()


# ---- td_flux_rope_table ------------------------------------------------------------------------------------------------------------

def _rope_table_f64(ids, axes, theta):
    """cos / sin float64 [S, 128] of FluxPosEmbed: axis a with d_a channels, freq_j = theta^(-2j / d_a), angle = id_a * freq_j, each value
    twice (columns 2j, 2j + 1)."""
    pos = ids.double()
    cs, sn = [], []
    for a, d in enumerate(axes):
        if d == 0:
            continue
        freq = 1.0 / (float(theta) ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
        ang = torch.outer(pos[:, a], freq)
        cs.append(ang.cos().repeat_interleave(2, dim=1))
        sn.append(ang.sin().repeat_interleave(2, dim=1))
    return torch.cat(cs, dim=1), torch.cat(sn, dim=1)


def _table_ids(S, kind):
    g = torch.Generator().manual_seed(S)
    if kind == "zeros":
        return torch.zeros(S, 3)
    if kind == "integer":
        ids = torch.randint(0, 4096, (S, 3), generator=g).float()
        ids[0] = torch.tensor([4095.0, 0.0, 4095.0])
        return ids
    if kind == "fractional":
        return torch.rand(S, 3, generator=g) * 300.0 + 0.37
    return -(torch.rand(S, 3, generator=g) * 200.0) - torch.randint(0, 50, (S, 3), generator=g).float()


@pytest.mark.parametrize("S", [1, 5, 261])
@pytest.mark.parametrize("theta", [1e4, 1e6])
@pytest.mark.parametrize("axes", [(16, 56, 56), (32, 48, 48), (0, 64, 64)])
def test_flux_rope_table_vs_float64(hip, axes, theta, S):
    """The kernel evaluates pow, the product, cos and sin in fp64 and rounds once to fp32, so every entry is within one fp32 ulp at
    magnitude 1 (2^-23) of float64 -- half an ulp of the rounding plus what fp64 pow / cos / sin of angles up to 4095 are off by
    (below 1e-12).  Ids: zeros, integers up to 4095, fractional, negative.  The pair columns 2j and 2j + 1 are equal bit for bit.
    261 rows x 64 pairs = 66 blocks and a partial one."""
    worst = 0.0
    for kind in ("zeros", "integer", "fractional", "negative"):
        ids = _table_ids(S, kind)
        cos, sin = hip.flux_rope_table(ids.cuda(), axes_dims=axes, theta=theta)
        torch.cuda.synchronize()
        rc, rs = _rope_table_f64(ids, axes, theta)
        tol = torch.full_like(rc, 2.0 ** -23)
        what = f"flux_rope_table axes={axes} theta={theta:g} S={S} ids={kind}"
        worst = max(worst, C._check(cos, rc, tol, what + " cos"), C._check(sin, rs, tol, what + " sin"))
        for t in (cos.cpu(), sin.cpu()):
            assert torch.equal(t[:, 0::2].view(torch.int32), t[:, 1::2].view(torch.int32)), what + ": pair columns differ"
        if kind == "zeros":
            assert torch.equal(cos.cpu(), torch.ones(S, 128)) and torch.equal(sin.cpu(), torch.zeros(S, 128))
    assert worst <= 1.0
    C.record(f"flux_rope_table[axes={'-'.join(map(str, axes))},theta={theta:g},S={S}]", worst)


def test_flux_rope_table_refuses_axes_that_do_not_sum_to_128(hip):
    ids = torch.zeros(4, 3, device="cuda")
    for axes in [(16, 56, 48), (16, 56, 64), (0, 0, 0)]:
        with pytest.raises(hip.ThinkDiffHipError, match="sum to 128"):
            hip.flux_rope_table(ids, axes_dims=axes)


# ---- td_timestep_sincos ------------------------------------------------------------------------------------------------------------

def test_timestep_sincos_vs_float64(hip):
    """out = [cos(t f_j) | sin(t f_j)], f_j = exp(-ln(1e4) j / 128), against float64 of the same formula on the fp32 t.  Bound per element:
    one bf16 ulp of the reference plus |t f_j| * 8 * 2^-24.  The second term is the fp32 angle: the constant ln(1e4) (half an ulp), its
    product with j, the division by 128 (exact), expf (1 ulp; its argument's error of up to 9.2 * 2^-24 absolute is what costs most), the
    product with t, and the device's sinf / cosf (1 - 2 ulps of a value <= 1 after an exact argument reduction) -- each a relative error of
    the angle of about 2^-24, and d/da of sin and cos is at most 1.  The build has no fast-math."""
    g = torch.Generator().manual_seed(5)
    t = torch.cat([torch.tensor([0.0, 12.25, 968.0, 1000.0, 3504.0]), torch.rand(300, generator=g) * 1000.0]).float()
    out = hip.timestep_sincos(t.cuda())
    torch.cuda.synchronize()
    j = torch.arange(128, dtype=torch.float64)
    ang = t.double()[:, None] * torch.exp(-math.log(10000.0) * j / 128.0)[None, :]
    ref = C.bf(torch.cat([ang.cos(), ang.sin()], dim=1))
    tol = C._ulp(ref) + torch.cat([ang, ang], dim=1).abs() * 8 * 2.0 ** -24
    worst = C._check(out, ref, tol, "timestep_sincos")
    assert torch.equal(C.bits(out[0]), C.bits(torch.cat([torch.ones(128), torch.zeros(128)]).bfloat16())), "t = 0 is not [1 | 0]"
    assert worst <= 1.0
    C.record("timestep_sincos", worst)


# ---- td_fill_normal_bf16 / td_fill_normal_from_bf16 ---------------------------------------------------------------------------

SEED = 0x1234_5678_9ABC_DEF1


@pytest.mark.parametrize("std,mean", [(1.0, 0.0), (0.05, 1.0)])
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_fill_normal_vs_generator(hip, n, std, mean):
    """Every element against the documented generator restated in numpy uint64 / float64 (flux_rowops_common.fill_normal_ref): within one
    bf16 ulp plus 16 * 2^-24 (|mean| + std r) -- the fp32 chain logf, the product with -2, sqrtf (r: about 3 ulps), the angle 2 pi u2
    rounded to fp32 (up to 4 * 2^-24 absolute in [4, 8)), sincosf (2 ulps), and the two products and the sum.  n is odd: the last pair
    writes one element and the element behind n keeps its sentinel.  4097 elements = 2049 pairs: nine blocks, the last with one lane."""
    buf = torch.full((n + 1,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hip.fill_normal(buf[:n], SEED, std=std, mean=mean)
    torch.cuda.synchronize()
    assert float(buf[n]) == SENTINEL, "the element behind n was written"
    v, r = C.fill_normal_ref(n, SEED, std, mean)
    ref = C.bf(v)
    tol = C._ulp(ref) + 16 * 2.0 ** -24 * (abs(mean) + std * r)
    worst = C._check(buf[:n].reshape(1, n), ref.reshape(1, n), tol.reshape(1, n), f"fill_normal n={n} std={std} mean={mean}")
    assert worst <= 1.0
    C.record(f"fill_normal[n={n},std={std},mean={mean}]", worst)


def test_fill_normal_seeds_and_pieces(hip):
    """Two seeds give different draws; td_fill_normal_from_bf16 with pair0 = k on a piece gives elements 2k .. of the whole fill bit for
    bit (an odd-length piece included); its draws follow the generator at pair0 + p; a negative pair0 is refused."""
    n = 4097
    whole = hip.fill_normal(torch.empty(n, dtype=torch.bfloat16, device="cuda"), SEED)
    other = hip.fill_normal(torch.empty(n, dtype=torch.bfloat16, device="cuda"), SEED + 1)
    torch.cuda.synchronize()
    assert int((C.bits(whole) != C.bits(other)).sum()) > n * 0.98
    for k, m in [(0, n), (1, 7), (300, 1025), (2048, 1), (1000, 2000)]:
        piece = torch.full((m + 1,), SENTINEL, dtype=torch.bfloat16, device="cuda")
        hip.fill_normal_from(piece[:m], SEED, k)
        torch.cuda.synchronize()
        assert torch.equal(C.bits(piece[:m]), C.bits(whole[2 * k: 2 * k + m])), f"pair0={k}, {m} elements"
        assert float(piece[m]) == SENTINEL
    # far beyond any whole fill a test can afford: pair0 = 2^33 against the generator
    k, m = 2 ** 33, 255
    piece = hip.fill_normal_from(torch.empty(m, dtype=torch.bfloat16, device="cuda"), SEED, k, std=0.05, mean=1.0)
    torch.cuda.synchronize()
    v, r = C.fill_normal_ref(m, SEED, 0.05, 1.0, pair0=k)
    ref = C.bf(v)
    worst = C._check(piece.reshape(1, m), ref.reshape(1, m), (C._ulp(ref) + 16 * 2.0 ** -24 * (1.0 + 0.05 * r)).reshape(1, m), "fill_normal_from pair0=2^33")
    assert worst <= 1.0
    C.record("fill_normal_from[pair0=2^33]", worst)
    L = hip.lib()
    assert L.td_fill_normal_from_bf16(hip.ptr(piece), m, SEED, 1.0, 0.0, -1, None) == 2 and b"pair0" in L.td_last_error()
    assert L.td_fill_normal_from_bf16(None, m, SEED, 1.0, 0.0, 0, None) == 2
    assert L.td_fill_normal_from_bf16(hip.ptr(piece), 0, SEED, 1.0, 0.0, 0, None) == 2
