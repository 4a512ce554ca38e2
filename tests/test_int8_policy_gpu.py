"""Kernel-level coverage of the 8-bit policy bench.py measures by default (int8 block Linears, history scales, per-channel smoothing with replicated
outlier channels, e4m3 joint attention), through the "int8 policy building blocks" entries of include/thinkdiff_hip.h.  tests/test_int8_gpu.py grades
the same kernels end to end with statistical bars; here every operation is compared with its exact integer statement.

Every reference does its quantisation arithmetic in fp32 torch on the CPU, exactly as the kernels state it:
    s = amax * (1.0f / 127)   (448 for e4m3; 1 where amax == 0)      inv = 1.0f / s      q = clamp(rint(v * inv), +-127), round half to even

Bars
 (a) norm -> int8, (b) row quantiser, (c) td_col_amax_bf16, (e) td_q8_scales_from_amax, (f) td_ext_cols_int8: EXACT equality of every byte, scale
     and accumulator bit, pad bytes and guard rows included.  (a) takes this project's own td_norm_rows_bf16 output of the same arguments as the row
     to quantise (the norm's arithmetic has its own tests); v = y * smooth is a product of two bf16 values, exact in fp32.
 (d) td_smooth_factors: exact equality with 2^clamp(rint(0.5 log2(ax / aw)), +-8) evaluated in fp64.  The device's log2f may be off by an ulp, so
     the maxima are drawn with 0.5 log2(ax / aw) at least 1e-3 away from every half-integer (asserted on the CPU), plus ratios that are exact powers of
     four (an exact integer exponent): on these inputs the fp64 statement is unambiguous.
 (g) int8 GEMM with int8 output: reference from the exact integer contraction, y = acc xs ws + b in fp64, t = bf16(y), a = bf16(act(t)),
     v = a smooth[n], q = clamp(rint(fp32(v) inv[m]), +-127), amax[m] = max(previous, max_n |v|).  The kernel dequantises in fp32 and evaluates GELU
     with the hardware's exp2 / rcp, so next to a bf16 tie t or a may round the other way -- one bf16 ulp, 2^-8 relative, i.e. at most one step
     of a byte (|q| <= 127).  Bars: EVERY byte within 1 step; at most 1e-3 of the bytes unequal; at most 1 % of the rows with another amax, those by
     one bf16 ulp.  (Two valid fp32 orderings of the dequantisation differ from the fp64 one in at most 4.8e-5 of the bf16 values and 4.4e-6 of the
     bytes when both are evaluated on a CPU: the cap is ~200x what a correct kernel needs, and a wrong column, row or scale breaks it by orders of magnitude.)
     The bf16 first output of the split form: within 2^-7 of the largest value, tests/test_int8_gpu.py's bar.
 (h) attention with int8 output: the same launch run twice, once with the bf16 output o, once with q8; q = clamp(rint(fp32(o) inv[row]), +-127) over
     all heads of a row, amax[row] = max(previous, max |o[row, :]|).  The bars of (g); zero mismatches are expected since both launches round the same
     fp32 values.

Measured on an MI355X (every case prints its counts before it asserts, `pytest -s`; summed over the outputs of each form)
 (g) plain   192 outputs: 4 of 12 960 000 bytes unequal (3.1e-7), each by 1 step, one in each of 4 outputs (cfg 0 and 2, M 258 and 300, N 768, K 256, no
             activation, no smoothing; worst output 1 of 198 144 = 5.1e-6, 200x under the cap); 0 of 30 000 rows with another amax
     split    16 outputs: 0 of 1 121 280 bytes unequal, 0 of 2 920 rows with another amax; the bf16 half inside its bar
     grouped  16 outputs: 0 of 1 300 000 bytes unequal, 0 of 2 500 rows with another amax
 (h) td_attention_q8 plain, td_attention_q8 pre-scaled / bounded, td_attention_fp8_q8: each 0 of 10 554 880 bytes unequal and 0 of 1 813 rows with
     another amax over its four shapes
 (a) - (f): every byte, scale and accumulator equal, as the bars ask.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 0x5A                      # what pad bytes and guard rows are pre-filled with


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _scale_ref(amax, qmax):
    """s = amax * (1.0f / qmax) in fp32, 1 for a zero row."""
    return torch.where(amax > 0, amax * (_f32(1.0) / _f32(qmax)), torch.ones_like(amax))


def _q_ref(v, inv):
    """clamp(rint(v * inv[row]), +-127): fp32 product, round half to even."""
    return torch.round(v * inv[:, None]).clamp(-127, 127).to(torch.int8)


def _quant_rows_ref(v, int8=True):
    """The row quantiser on fp32 values v [R, K] (CPU): (bytes, scale, row maxima)."""
    amax = v.abs().amax(dim=1)
    s = _scale_ref(amax, 127.0 if int8 else 448.0)
    inv = _f32(1.0) / s
    if int8:
        return _q_ref(v, inv), s, amax
    return (v * inv[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), s, amax


def _bits(t):
    """float32 -> int32 bit patterns (what the maxima accumulators hold)."""
    return t.contiguous().view(torch.int32)


def _bytes_buffer(rows, ld, dtype=torch.int8, guard=2):
    """[rows + guard, ld] bytes pre-filled with PAD; the kernels get the first `rows` rows."""
    return torch.full((rows + guard, ld), PAD, dtype=dtype, device="cuda")


# ---- (a) norm -> int8 with smoothing and replicated channels ---------------------------------------------------------------------------------
def _ext_table(g, n, D, variant):
    t = torch.randint(0, D, (n,), generator=g, dtype=torch.int32)
    if n == 2:
        return torch.tensor([D - 1, D - 1] if variant == 0 else [-1, 0], dtype=torch.int32)
    t[torch.randperm(n, generator=g)[: max(1, n // 8)]] = -1
    t[0] = D - 1                                   # the last channel
    t[1] = t[2] = t[3] = D // 2                    # a source repeated three times
    t[n - 1] = -1 if variant == 0 else 5           # the table's last entry (the one the kernel's tail loop writes for ext_n = 130)
    return t


@pytest.mark.parametrize("form", ["layernorm_mod", "rmsnorm_w"])
@pytest.mark.parametrize("D", [512, 1536, 3072, 4096])
def test_norm_rows_quant_int8_bit_exact(hip, D, form):
    g = torch.Generator().manual_seed(D + len(form))
    rms = form == "rmsnorm_w"
    mods = [(torch.randn(D, generator=g) * 0.3).bfloat16().cuda() for _ in range(4)]
    w = (1.0 + 0.2 * torch.randn(D, generator=g)).bfloat16().cuda()
    smooth = {"pow2": [torch.exp2(-torch.randint(0, 9, (D,), generator=g).float()).bfloat16().cuda() for _ in range(2)],       # 2^-8 .. 1
              "any": [(torch.rand(D, generator=g) * 1.5 + 0.01).bfloat16().cuda() for _ in range(2)]}
    ext = {n: [_ext_table(g, n, D, v).cuda() for v in range(2)] for n in (2, 64, 128, 130, 256)}
    assert not torch.equal(ext[64][0], ext[64][1]) and int(ext[130][0][0]) == D - 1 and int(ext[130][0][129]) == -1
    n_cases = 0
    for rows in (1, 3, 5, 257):
        x = (torch.randn(rows, D, generator=g) * torch.logspace(-2, 2, rows)[:, None]).bfloat16()
        x[:, 7] *= 30.0                              # an outlier channel
        if rows >= 3:
            x[1] = 0                                 # an all-zero row
        x = x.cuda()
        for split in sorted({0, min(2, rows), rows}):
            kw = dict(rms=True, eps=1e-6, w=w) if rms else dict(rms=False, eps=1e-6, split=split, shiftA=mods[0], scaleA=mods[1], shiftB=mods[2], scaleB=mods[3])
            y = hip.norm_rows(x, **kw)
            q0, s0 = hip.norm_rows_quant8(x, split=split, **{k: v for k, v in kw.items() if k != "split"})
            qq, sq = hip.quant_rows_int8(y)
            torch.cuda.synchronize()
            assert torch.equal(q0, qq) and torch.equal(s0, sq), "without smoothing and ext: the bytes of td_quant_rows_int8(y)"
            yc = y.float().cpu()
            partB = (torch.arange(rows) >= split)[:, None]
            for sm_kind, (smA, smB) in smooth.items():
                v = yc * torch.where(partB, smB.float().cpu()[None, :], smA.float().cpu()[None, :])
                q_want, s_want, _ = _quant_rows_ref(v)
                if rms and rows >= 3:
                    assert float(s_want[1]) == 1.0 and not q_want[1].any()
                # the e4m3 form takes the same smoothing factors (and no ext tables): bytes and scales under max / 448
                f_want, fs_want, _ = _quant_rows_ref(v, int8=False)
                buf = _bytes_buffer(rows, D + 16, torch.uint8)
                _, s = hip.norm_rows_quant8(x, int8=False, q=buf[:rows], split=split, smoothA=smA, smoothB=smB, **{k: v for k, v in kw.items() if k != "split"})
                torch.cuda.synchronize()
                want = torch.full((rows + 2, D + 16), PAD, dtype=torch.uint8)
                want[:rows, :D] = f_want
                assert torch.equal(s.cpu(), fs_want), (rows, split, sm_kind, "e4m3")
                assert torch.equal(buf.cpu(), want), (rows, split, sm_kind, "e4m3", (buf.cpu() != want).nonzero()[:8].tolist())
                n_cases += 1
                for n, (eA, eB) in ext.items():
                    ldq = (D + n + 7) // 8 * 8 + 16
                    buf = _bytes_buffer(rows, ldq)
                    _, s = hip.norm_rows_quant8(x, q=buf[:rows], split=split, smoothA=smA, smoothB=smB, extA=eA, extB=eB, **{k: v for k, v in kw.items() if k != "split"})
                    torch.cuda.synchronize()
                    got = buf.cpu()
                    want = torch.full_like(got, PAD)
                    want[:rows, :D] = q_want
                    src = torch.where(partB, eB.cpu()[None, :], eA.cpu()[None, :]).long()
                    want[:rows, D:D + n] = torch.where(src >= 0, torch.gather(q_want, 1, src.clamp(min=0)), torch.zeros((), dtype=torch.int8))
                    assert torch.equal(s.cpu(), s_want), (rows, split, sm_kind, n)
                    bad = (got != want).nonzero()
                    assert bad.numel() == 0, (rows, split, sm_kind, n, bad[:8].tolist())
                    n_cases += 1
    print(f"norm -> int8 D={D} {form}: {n_cases} launches bit-exact")


# ---- (b) row quantiser with col_mul / amax_out ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 520, 3072, 3200, 12288])
def test_quant_rows8_bit_exact(hip, K):
    g = torch.Generator().manual_seed(K)
    col_mul = (torch.exp2(torch.randint(-8, 9, (K,), generator=g).float()) * (1.0 + 0.5 * torch.rand(K, generator=g))).cuda()       # arbitrary fp32 factors
    for rows in (1, 5, 77):
        ldx, ldq = K + 24, K + 40
        xw = (torch.randn(rows, ldx, generator=g) * torch.logspace(-3, 2, rows)[:, None]).bfloat16()
        if rows >= 5:
            xw[3, :K] = 0                                # a zero row (its pad columns are not)
            xw[2, K - 1] = -3.0e4                        # the row maximum in the last column, negative
        xw = xw.cuda()
        x = xw[:, :K]
        for int8 in (True, False):
            for cm in (None, col_mul):
                buf = _bytes_buffer(rows, ldq, torch.int8 if int8 else torch.uint8)
                _, s, amax = hip.quant_rows8(x, int8=int8, col_mul=cm, want_amax=True, q=buf[:rows, :K])
                torch.cuda.synchronize()
                v = x.float().cpu() * (cm.cpu()[None, :] if cm is not None else 1.0)
                q_want, s_want, amax_want = _quant_rows_ref(v, int8)
                want = torch.full((rows + 2, ldq), PAD, dtype=q_want.dtype)
                want[:rows, :K] = q_want
                assert torch.equal(s.cpu(), s_want), (rows, int8, cm is not None)
                assert torch.equal(amax.cpu(), _bits(amax_want)), (rows, int8, cm is not None)
                assert torch.equal(buf.cpu(), want), (rows, int8, cm is not None)
                if rows >= 5:
                    assert float(s[3]) == 1.0 and not buf[3, :K].any()
                if int8:
                    assert int(buf[:rows, :K].abs().max()) == 127 and int(buf[:rows, :K].min()) >= -127


# ---- (c) td_col_amax_bf16 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 2048, 2056, 3072])
def test_col_amax_bit_exact(hip, K):
    g = torch.Generator().manual_seed(K + 1)
    for rows in (1, 63, 64, 65, 300):
        ldx = K + 8
        xw = (torch.randn(rows, ldx, generator=g) * torch.logspace(-2, 2, K + 8)[None, :]).bfloat16()
        xw[:, 0] = -xw[:, 0].abs()                       # an all-negative column
        xw[:, min(3, K - 1)] = 0                         # a column of zeros ...
        xw[::2, min(3, K - 1)] = -0.0                    # ... of both signs
        xw = xw.cuda()
        x = xw[:, :K]
        colmax = x.float().abs().amax(dim=0).cpu()
        prev = colmax.clone()
        prev[0::3] *= 2.0                                # above the column's maximum
        prev[1::3] *= 0.5                                # below it
        prev[2::3] = 0.0                                 # an empty accumulator
        prev[min(3, K - 1)] = 0.375                      # the zero column's accumulator must stay as it was
        want = _bits(torch.maximum(prev, colmax))
        acc = torch.full((K + 8,), PAD, dtype=torch.int32)
        acc[:K] = _bits(prev)
        one = hip.col_amax(x, acc.cuda()[:K].clone())
        two = acc.cuda()[:K].clone()
        if rows > 1:
            hip.col_amax(x[:rows // 2], two)
            hip.col_amax(x[rows // 2:], two)
        else:
            hip.col_amax(x, two)
        guarded = acc.cuda()
        hip.col_amax(x, guarded[:K])
        torch.cuda.synchronize()
        assert torch.equal(one.cpu(), want), (rows, (one.cpu() != want).nonzero()[:8].tolist())
        assert torch.equal(two.cpu(), want), rows
        assert torch.equal(guarded.cpu()[:K], want) and bool((guarded.cpu()[K:] == PAD).all())
        assert int(one[min(3, K - 1)]) == int(_bits(_f32([0.375]))[0])


# ---- (d) td_smooth_factors --------------------------------------------------------------------------------------------------------------------
def test_smooth_factors_exact(hip):
    g = torch.Generator().manual_seed(11)
    n_rand = 4000
    aw = torch.exp2(torch.rand(n_rand, generator=g) * 20 - 10)
    ax = aw * torch.exp2(torch.rand(n_rand, generator=g) * 44 - 22)                 # 0.5 log2(ax / aw) in (-11, 11): both clamps are reached
    e = 0.5 * torch.log2(ax.double() / aw.double())
    keep = ((e - torch.floor(e)) - 0.5).abs() >= 2e-3                               # at least 1e-3 (doubled for slack) away from every half-integer
    ax, aw = ax[keep], aw[keep]
    k = torch.arange(-12, 13).float()
    base = torch.tensor([0.0137, 1.0, 3.25, 900.0])
    ax = torch.cat([ax, (base[:, None] * torch.exp2(2 * k)[None, :]).flatten(), torch.tensor([0.0, 2.5, 0.0])])     # exact powers of four; zeros
    aw = torch.cat([aw, base[:, None].expand(4, 25).flatten(), torch.tensor([1.5, 0.0, 0.0])])
    n = ax.numel()
    assert n % 256 != 0 and n > 1024
    pos = (ax > 0) & (aw > 0)
    e = torch.where(pos, 0.5 * torch.log2(ax.double().clamp(min=1e-300) / aw.double().clamp(min=1e-300)), torch.zeros(n, dtype=torch.float64))      # (a power-of-two ratio: exact)
    dist = ((e - torch.floor(e)) - 0.5).abs()
    assert bool((dist[pos] >= 1e-3).all()), "the drawn maxima must keep 0.5 log2(ax / aw) away from the half-integers"
    exact = e[n_rand - int((~keep).sum()):n - 3]
    assert bool((exact == torch.round(exact)).all())                                 # the powers of four: exact integer exponents
    ee = torch.round(e).clamp(-8, 8)
    assert bool((ee == -8).any()) and bool((ee == 8).any()) and bool((torch.round(e) < -8).any()) and bool((torch.round(e) > 8).any())
    s_want = torch.exp2(ee).float()
    s, inv, inv16 = hip.smooth_factors(_bits(ax).cuda(), _bits(aw).cuda())
    torch.cuda.synchronize()
    assert torch.equal(s.cpu(), s_want), (s.cpu() != s_want).nonzero()[:8].tolist()
    assert torch.equal(inv.cpu(), 1.0 / s_want) and torch.equal(inv16.cpu(), (1.0 / s_want).bfloat16())
    assert s_want[-3:].tolist() == [1.0, 1.0, 1.0]


# ---- (e) td_q8_scales_from_amax ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 70000])
def test_q8_scales_from_amax_bit_exact(hip, n):
    g = torch.Generator().manual_seed(n)
    a = torch.exp2(torch.rand(n, generator=g) * 30 - 15) * (1.0 + torch.rand(n, generator=g))
    a[::7] = 0.0                                         # rows without history
    for margin in (1.0, 1.25):
        acc = torch.full((n + 8,), PAD, dtype=torch.int32)
        acc[:n] = _bits(a)
        acc = acc.cuda()
        scale, inv = hip.q8_scales_from_amax(acc[:n], margin)
        torch.cuda.synchronize()
        s_want = torch.where(a > 0, a * _f32(margin) * (_f32(1.0) / _f32(127.0)), torch.ones(n))
        assert torch.equal(scale.cpu(), s_want) and torch.equal(inv.cpu(), _f32(1.0) / s_want)
        assert float(scale[0]) == 1.0 and float(inv[0]) == 1.0
        assert not acc[:n].any() and bool((acc[n:] == PAD).all()), "every accumulator is cleared, nothing behind them is touched"
    with pytest.raises(hip.ThinkDiffHipError):
        hip.q8_scales_from_amax(_bits(a).cuda(), 0.99)


# ---- (f) td_ext_cols_int8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext_n", [2, 64, 130])
def test_ext_cols_bit_exact(hip, ext_n):
    g = torch.Generator().manual_seed(ext_n)
    for rows in (1, 5, 300):
        for K in (64, 3072):
            ld = K + ext_n + 22
            ext = _ext_table(g, ext_n, K, rows % 2)
            q = torch.randint(-127, 128, (rows + 2, ld), generator=g, dtype=torch.int8)
            want = q.clone()
            want[:rows, K:K + ext_n] = torch.where(ext[None, :] >= 0, q[:rows][:, ext.long().clamp(min=0)], torch.zeros((), dtype=torch.int8))
            d = q.cuda()
            hip.ext_cols_int8(d[:rows], K, ext.cuda())
            torch.cuda.synchronize()
            assert torch.equal(d.cpu(), want), (rows, K, (d.cpu() != want).nonzero()[:8].tolist())


# ---- (g) int8 GEMM with int8 output -----------------------------------------------------------------------------------------------------------
def _gelu_tanh64(t):
    return 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)))


class _GemmData:
    """Operands and exact integer contractions, made once for the largest extents and sliced by every case (rows of x and of w are independent)."""

    def __init__(self):
        g = torch.Generator().manual_seed(21)
        self.M, self.N = 300, 768
        self.K = {}
        for K in (256, 1024):
            d = {}
            for name, M in (("a", 300), ("b", 65)):      # problem 0 and the second problem of the grouped launches
                d["xq" + name] = torch.randn(M, K, generator=g).mul(40).round().clamp(-127, 127).to(torch.int8)
                d["wq" + name] = torch.randn(self.N, K, generator=g).mul(40).round().clamp(-127, 127).to(torch.int8)
                d["xs" + name] = (0.5 + torch.rand(M, generator=g)) / 40
                d["ws" + name] = 0.05 * (0.5 + torch.rand(self.N, generator=g)) / 40
                d["b" + name] = torch.randn(self.N, generator=g).bfloat16()
                acc = d["xq" + name].double() @ d["wq" + name].double().T                                   # exact: |sum| < 2^31
                d["y" + name] = acc * d["xs" + name].double()[:, None] * d["ws" + name].double()[None, :] + d["b" + name].double()[None, :]
                d["sm" + name] = torch.exp2(torch.randint(-6, 7, (self.N,), generator=g).float()).bfloat16()     # distinct powers of two per column
            self.K[K] = d


@pytest.fixture(scope="module")
def gemm_data():
    return _GemmData()


def _q8_reference(y, act, smooth, M, n0, n1):
    """v of the issue's statement for rows [0, M), columns [n0, n1) of the fp64 Linear output y: bf16(act(bf16(y))) * smooth[n], in fp32."""
    t = y[:M, n0:n1].to(torch.bfloat16)
    a = _gelu_tanh64(t.double()).to(torch.bfloat16) if act else t
    return a.float() * (smooth[n0:n1].float()[None, :] if smooth is not None else 1.0)


def _q8_scales(v, g):
    """Per-row inverse scales from three sources (row m: m % 3) and pre-loaded maxima; all fp32 CPU."""
    M = v.shape[0]
    vmax = v.abs().amax(dim=1)
    own = _f32(1.0) / torch.where(vmax > 0, vmax * _f32(1.25) * (_f32(1.0) / _f32(127.0)), torch.ones(M))     # the row's own maximum x 1.25 (td_q8_scales_from_amax)
    inv = torch.where(torch.arange(M) % 3 == 0, own, torch.where(torch.arange(M) % 3 == 1, own * 4.0, torch.ones(M)))      # x 4: a scale four times too small; 1: no history
    above = (vmax * 2.0 + 1.0).bfloat16().float()               # (a bf16 value, as every maximum the kernels accumulate is)
    prev = torch.where(torch.arange(M) % 4 == 0, above, torch.where(torch.arange(M) % 4 == 1, vmax * 0.25, torch.zeros(M)))
    return inv, prev


def _check_q8(tag, got_q, got_amax, v, inv, prev, M, n, stats):
    """The bars of (g) / (h) on one int8 output: got_q [M + guard, ld] bytes (CPU), got_amax int32 bits [M + guard]."""
    want_q = _q_ref(v, inv)
    want_amax = torch.maximum(prev, v.abs().amax(dim=1))
    assert bool((got_q[:M, n:] == PAD).all()) and bool((got_q[M:] == PAD).all()), f"{tag}: pad bytes / guard rows overwritten"
    assert bool((got_amax[M:] == PAD).all()), f"{tag}: maxima behind the last row overwritten"
    d = (got_q[:M, :n].int() - want_q.int()).abs()
    n_bad = int((d != 0).sum())
    wb = _bits(want_amax)
    rows_bad = int((got_amax[:M] != wb).sum())
    ga, wa = got_amax[:M] >> 16, wb >> 16                        # bf16 bit patterns (every v is a bf16 value times a power of two: the low halves are 0)
    low_ok = bool(((got_amax[:M] & 0xffff) == (wb & 0xffff)).all())
    stats.append((tag, n_bad, M * n, rows_bad, M))
    print(f"{tag}: {n_bad} of {M * n} bytes unequal ({n_bad / (M * n):.2e}), max step {int(d.max())}, {rows_bad} of {M} rows with another amax")
    assert int(got_q[:M, :n].min()) >= -127, f"{tag}: -128 where -127 belongs"
    assert int(d.max()) <= 1, f"{tag}: a byte {int(d.max())} steps off at {(d > 1).nonzero()[:8].tolist()}"
    assert n_bad <= 1e-3 * M * n, f"{tag}: {n_bad} of {M * n} bytes unequal, first at {(d != 0).nonzero()[:8].tolist()}"
    assert low_ok and rows_bad <= 0.01 * M and int((ga - wa).abs().max()) <= 1, f"{tag}: {rows_bad} of {M} row maxima differ, rows {(got_amax[:M] != wb).nonzero()[:8].flatten().tolist()}"
    return want_q


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("N", [256, 272, 768])
@pytest.mark.parametrize("M", [2, 65, 258, 300])
@pytest.mark.parametrize("cfg", [0, 2])
def test_linear_int8_q8_output(hip, gemm_data, cfg, M, N, K):
    d = gemm_data.K[K]
    g = torch.Generator().manual_seed(cfg + M + N + K)
    xq, xs = d["xqa"][:M].cuda(), d["xsa"][:M].cuda()
    wq, ws, b = d["wqa"][:N].contiguous().cuda(), d["wsa"][:N].cuda(), d["ba"][:N].cuda()
    ldq8 = N + 48
    stats, saturated = [], False
    for act in (hip.ACT_NONE, hip.ACT_GELU_TANH):
        for smooth in (None, d["sma"][:N]):
            v = _q8_reference(d["ya"], act, smooth, M, 0, N)
            inv, prev = _q8_scales(v, g)
            buf = _bytes_buffer(M, ldq8)
            amax = torch.full((M + 2,), PAD, dtype=torch.int32)
            amax[:M] = _bits(prev)
            amax = amax.cuda()
            pr = hip.q8_problem(xq, xs, wq, ws, b, buf, inv.cuda(), amax, smooth.cuda() if smooth is not None else None)
            hip.linear_int8_q8(pr, N, K, ldx=K, ldq8=ldq8, act=act, tile_cfg=cfg)
            torch.cuda.synchronize()
            want_q = _check_q8(f"gemm cfg{cfg} M{M} N{N} K{K} act{act} smooth{int(smooth is not None)}", buf.cpu(), amax.cpu(), v, inv, prev, M, N, stats)
            sat = want_q[1::3]
            saturated |= bool((sat == 127).any() and (sat == -127).any()) and bool((buf[1:M:3, :N] == 127).any() and (buf[1:M:3, :N] == -127).any())
    assert saturated, "the scale four times too small must drive bytes to +127 and -127"
    with pytest.raises(hip.ThinkDiffHipError):
        hip.linear_int8_q8(pr, N, K, ldx=K, ldq8=ldq8, act=hip.ACT_NONE, tile_cfg=3)


@pytest.mark.parametrize("n_split", [256, 512])
@pytest.mark.parametrize("M", [65, 300])
@pytest.mark.parametrize("cfg", [0, 2])
def test_linear_split_int8_q8_output(hip, gemm_data, cfg, M, n_split):
    """[bf16 | int8] outputs of one launch (the single-stream block's [q k v | mlp] projection): the int8 half's smoothing is indexed by the absolute column."""
    N, K = 768, 256
    d = gemm_data.K[K]
    g = torch.Generator().manual_seed(cfg + M + n_split)
    xq, xs, wq, ws, b = d["xqa"][:M].cuda(), d["xsa"][:M].cuda(), d["wqa"].cuda(), d["wsa"].cuda(), d["ba"].cuda()
    n8 = N - n_split
    ldq8 = n8 + 512
    stats = []
    for smooth in (None, d["sma"]):
        v = _q8_reference(d["ya"], True, smooth, M, n_split, N)
        inv, prev = _q8_scales(v, g)
        buf = _bytes_buffer(M, ldq8)
        amax = torch.full((M + 2,), PAD, dtype=torch.int32)
        amax[:M] = _bits(prev)
        amax = amax.cuda()
        y0 = torch.full((M + 2, n_split + 8), 7.0, dtype=torch.bfloat16, device="cuda")
        pr = hip.q8_problem(xq, xs, wq, ws, b, buf, inv.cuda(), amax, smooth.cuda() if smooth is not None else None)
        hip.linear_split_int8_q8(pr, N, K, ldx=K, ldq8=ldq8, y0=y0[:M, :n_split], act0=hip.ACT_NONE, act1=hip.ACT_GELU_TANH, n_split=n_split, tile_cfg=cfg)
        torch.cuda.synchronize()
        _check_q8(f"split cfg{cfg} M{M} n_split{n_split} smooth{int(smooth is not None)}", buf.cpu(), amax.cpu(), v, inv, prev, M, n8, stats)
        want0 = d["ya"][:M, :n_split].float()
        got0 = y0.float().cpu()
        assert bool((got0[M:] == 7.0).all()) and bool((got0[:, n_split:] == 7.0).all()), "bf16 output: pad columns / guard rows overwritten"
        err = float((got0[:M, :n_split] - want0).abs().max() / want0.abs().max())
        assert err < 2 ** -7, err


@pytest.mark.parametrize("N", [272, 768])
@pytest.mark.parametrize("M0,M1", [(300, 65), (258, 2)])
@pytest.mark.parametrize("cfg", [0, 2])
def test_linear_grouped2_int8_q8_output(hip, gemm_data, cfg, M0, M1, N):
    """Two problems in one launch, each with its own rows, weights, scales, maxima and smoothing factors."""
    K = 256
    d = gemm_data.K[K]
    g = torch.Generator().manual_seed(cfg + M0 + M1 + N)
    ldq8 = N + 16
    stats, probs, keep = [], [], []
    for name, M in (("a", M0), ("b", M1)):
        smooth = d["sm" + name][:N]
        v = _q8_reference(d["y" + name], True, smooth, M, 0, N)
        inv, prev = _q8_scales(v, g)
        buf = _bytes_buffer(M, ldq8)
        amax = torch.full((M + 2,), PAD, dtype=torch.int32)
        amax[:M] = _bits(prev)
        amax = amax.cuda()
        probs.append(hip.q8_problem(d["xq" + name][:M].cuda(), d["xs" + name][:M].cuda(), d["wq" + name][:N].contiguous().cuda(), d["ws" + name][:N].cuda(),
                                    d["b" + name][:N].cuda(), buf, inv.cuda(), amax, smooth.cuda()))
        keep.append((buf, amax, v, inv, prev, M))
    hip.linear_grouped2_int8_q8(probs[0], probs[1], N, K, ldx=K, ldq8=ldq8, act=hip.ACT_GELU_TANH, tile_cfg=cfg)
    torch.cuda.synchronize()
    for i, (buf, amax, v, inv, prev, M) in enumerate(keep):
        _check_q8(f"grouped cfg{cfg} ({M0},{M1}) N{N} problem{i}", buf.cpu(), amax.cpu(), v, inv, prev, M, N, stats)


# ---- (h) joint attention with int8 output -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["bf16", "bf16_prescaled_bounded", "fp8"])
@pytest.mark.parametrize("S,H", [(64, 1), (300, 2), (449, 4), (1000, 80)])
def test_attention_q8_output(hip, S, H, kernel):
    g = torch.Generator().manual_seed(S + H)
    W = H * 128
    qkv = torch.randn(S, 3 * W, generator=g).bfloat16()
    qkv[:, 2 * W:] = (qkv[:, 2 * W:].float() * torch.logspace(-1, 1, W)[None, :]).bfloat16()          # value columns of different magnitude
    bound = 0.0
    if kernel == "bf16_prescaled_bounded":
        qkv[:, :W] = (qkv[:, :W].float() * (128 ** -0.5 * 1.4426950408889634)).bfloat16()
        qh, kh = qkv[:, :W].float().view(S, H, 128), qkv[:, W:2 * W].float().view(S, H, 128)
        bound = min(48.0, float(qh.norm(dim=2).amax() * kh.norm(dim=2).amax()))                       # Cauchy-Schwarz over all rows and heads
    d = qkv.cuda()
    q, k, v = d[:, :W], d[:, W:2 * W], d[:, 2 * W:]
    o = torch.zeros(S, W, dtype=torch.bfloat16, device="cuda")
    if kernel == "bf16":
        hip.attention(q[None], k[None], v[None], o[None], H, H)
    elif kernel == "fp8":
        hip.attention_fp8(q, k, v, o, H)
    else:
        hip.attention_joint_prescaled(q, k, v, o, H, bound)
    torch.cuda.synchronize()
    oc = o.float().cpu()
    assert torch.isfinite(oc).all() and float(oc.abs().max()) > 0
    inv, prev = _q8_scales(oc, g)
    ldq8 = W + 512                                       # the [attn | mlp] row of the single-stream block
    buf = _bytes_buffer(S, ldq8)
    amax = torch.full((S + 2,), PAD, dtype=torch.int32)
    amax[:S] = _bits(prev)
    amax = amax.cuda()
    if kernel == "fp8":
        hip.attention_fp8_q8(q, k, v, buf[:S], inv.cuda(), amax[:S], H)
    else:
        hip.attention_q8(q, k, v, buf[:S], inv.cuda(), amax[:S], H, q_prescaled=kernel != "bf16", score_bound=bound)
    torch.cuda.synchronize()
    stats = []
    want_q = _check_q8(f"attention {kernel} S{S} H{H}", buf.cpu(), amax.cpu(), oc, inv, prev, S, W, stats)
    assert bool((want_q[1::3] == 127).any() and (want_q[1::3] == -127).any()), "the saturating scale must reach +-127"
    got_sat = buf[1:S:3, :W]
    assert bool((got_sat == 127).any() and (got_sat == -127).any()), "the kernel's bytes must reach +-127 under the saturating scale too"
