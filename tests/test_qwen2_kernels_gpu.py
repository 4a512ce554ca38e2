"""The Qwen2 side's small kernels, each against a plain restatement of its operation: the half-split rotary modes of
td_qk_norm_rope_bf16 (rotate_half = 1 and 2), td_mrope_table and td_embed_gather_bf16.  Every reference is computed on the CPU from
the bf16-valued inputs, with the kernel's documented rounding points (include/thinkdiff_hip.h, csrc/qk_rope_math.h) restated here.

Tolerances, per element (ulp(r) = one bf16 ulp of r, 2^(floor(log2 |r|) - 7)):

* rotate_half = 2, no norm weights: NONE, bit-exact.  y = bf16(bf16(x cos) + bf16(rot(x) sin)); each product and the sum is ONE fp32
  operation on bf16-valued (x) and fp32 (table) operands, rounded to bf16 before the next, so IEEE fp32 on the CPU gives the same bits
  and nothing can be contracted across a rounding.
* rotate_half = 1, no norm weights: y = bf16(x cos + rot(x) sin) as one fp32 expression, compared with float64:
  ulp(y) + 4 * 2^-24 (|x cos| + |x_partner sin|).  ulp(y) is the final rounding where the fp32 value sits next to a rounding boundary;
  the second term is two fp32 products and one sum (<= 3 roundings of 2^-24 relative to the larger operand), rounded up to 4.  Whether
  the compiler contracts a product into the sum is its choice, hence no bit-exactness.
* with norm weights (both modes): n = bf16(bf16(x rstd) w) before the rotation, rstd = rsqrt(mean x^2 + eps) in fp32.  One bf16 ulp at
  each rounding point, moved through the rotation:
  ulp(y) + |cos| (ulp(n_i) + |w_i| ulp(t_i)) + |sin| (ulp(n_p) + |w_p| ulp(t_p)), t = bf16(x rstd), p = the partner element i +- 64.
  The fp32 rstd (a 128-term sum and a hardware rsqrt, ~2^-22 relative) only matters where it flips the rounding of t: that flip is
  the |w| ulp(t) term.
* td_mrope_table, round_bf16 = 0, against float64 cos / sin(pos * theta^(-2j/128)):  4 * 2^-24 |angle| + 4 * 2^-24.  Derived, not
  measured, for an fp32 angle = pos * (1 / powf(theta, j/64)): two ulps for powf (the exponent j/64 and pos < 2^24 are exact), one for
  the reciprocal and one for the product -- 4 * 2^-24 relative, which moves cos / sin by that times |angle|; cosf / sinf of the fp32
  angle are good to a few ulps of 1 at any argument (full-precision argument reduction): 4 * 2^-24 absolute.  (The kernel now rounds
  the power correctly, through double: three roundings of 2^-24 each, inside the same bound.)
  round_bf16 = 1: half a bf16 ulp of the exact value (the rounding) plus the bound above, and every value bf16-representable.
  The structural properties (columns 64 + j = j, the sections' stream mapping, independence of the sections when the three streams
  are equal) are exact.
* td_embed_gather_bf16: a copy, bit-exact; ids outside [0, vocab) read row 0 / row vocab - 1 (the documented clamp).

Measured on MI355X (printed by the tests), max error x the bound: rotate_half = 1 without weights 1.000 (130 x 14 units: one element one
ulp(y) off, a flipped final rounding), 0.93, and 0 on the three small shapes; with weights 0.08 (mode 1) and 0 (mode 2: the same bits as
the float64 restatement); td_mrope_table round_bf16 = 0: cos 0.37 / sin 0.52 (theta 1e6), 0.37 / 0.41 (theta 1e4), the same for all four
section splits (every stream holds every position); round_bf16 = 1: 0.996 / 0.992 and 0.984 / 0.993.  Against the oracle's bf16 tables:
0 of 65536 elements differ (with powf in the kernel: 2.83 %, 0.87 % by more than one bf16 ulp -- test_mrope_table_vs_oracle_bf16).
"""
import numpy as np
import pytest
import torch

from oracle import qwen2vl_ref as Q

pytestmark = pytest.mark.gpu


def _ulp(r):
    a = r.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rot(x):
    """rotate_half on the last axis (128): cat(-x[64:], x[:64])."""
    return torch.cat((-x[..., 64:], x[..., :64]), dim=-1)


def _check(got, ref, tol, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    bad = err > tol
    ratio = err / tol
    print(f"{what}: max error {float(ratio.max()):.3f} x the bound")
    if bad.any():
        i = int(torch.argmax(ratio))
        idx = tuple(int(j) for j in np.unravel_index(i, tuple(ref.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements beyond the bound; worst {idx}: got {float(got[idx]):.6g} "
                             f"ref {float(ref[idx]):.6g} ({float(ratio[idx]):.3g} x the bound)")


# ---- td_qk_norm_rope_bf16, rotate_half = 1 and 2 --------------------------------------------------------------------------

# (rows, Hq, Hk): a block walks the Hq + Hk head-units of its row 16 per pass -- 3 units; 8 = half a pass; 14 = a partial pass;
# 20 = a partial second pass; 32 = two full passes (the Qwen2-VL-7B head counts)
ROPE_SHAPES = [(1, 2, 1), (37, 6, 2), (130, 12, 2), (64, 16, 4), (5, 28, 4)]


def _qwen_buffer(rows, Hq, Hk, seed):
    """The Qwen2 projection buffer [q(Hq) | k(Hk) | v(Hk)] + 64 pad columns, every head with its own scale."""
    g = torch.Generator().manual_seed(seed)
    W = (Hq + 2 * Hk) * 128
    buf = torch.randn(rows, W + 64, generator=g)
    buf[:, :W] *= (0.5 + torch.rand(Hq + 2 * Hk, generator=g)).repeat_interleave(128)
    return buf.bfloat16()


def _tables(rows, kind, seed):
    """fp32 cos / sin [rows, 128]: 'bf16' = the engine's (M-RoPE tables rounded to bf16, positions t != h != w up to 2^17);
    'fp32' = arbitrary fp32 values, the two halves of a row different (nothing may assume column 64 + j = column j)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "bf16":
        pos = torch.randint(0, 131072, (3, rows), generator=g)
        c, s = Q.mrope_cos_sin(pos, Q.Qwen2Config(), torch.bfloat16)
        return c.float().contiguous(), s.float().contiguous()
    ang = torch.rand(rows, 128, generator=g) * 6.2831853
    return torch.cos(ang).contiguous(), (torch.sin(ang) * (0.5 + torch.rand(rows, 128, generator=g))).contiguous()


def _heads(buf, rows, Hq, Hk):
    """q and k heads of the buffer as one [rows, Hq + Hk, 128] tensor (they are adjacent: k_col = Hq * 128)."""
    return buf[:, :(Hq + Hk) * 128].reshape(rows, Hq + Hk, 128)


@pytest.mark.parametrize("tables", ["bf16", "fp32"])
@pytest.mark.parametrize("rows,Hq,Hk", ROPE_SHAPES)
def test_rope_mode2_is_the_bf16_torch_graph_bit_for_bit(hip, rows, Hq, Hk, tables):
    """rotate_half = 2 (every Qwen2 prefill and decode step), no norm weights: the same bits as the torch graph on bf16 tensors,
    bf16(bf16(x cos) + bf16(rotate_half(x) sin)), restated in CPU fp32.  v and the pad columns keep their bits."""
    buf = _qwen_buffer(rows, Hq, Hk, rows * 7 + Hq)
    cos, sin = _tables(rows, tables, rows + Hk)
    x = _heads(buf, rows, Hq, Hk)
    a = (x.float() * cos[:, None, :]).bfloat16()
    b = (_rot(x).float() * sin[:, None, :]).bfloat16()
    want = (a.float() + b.float()).bfloat16()
    d = buf.cuda()
    hip.qk_norm_rope(d, Hq, Hk, 0, Hq * 128, cos.cuda(), sin.cuda(), rotate_half=2)
    torch.cuda.synchronize()
    got = d.cpu()
    diff = _bits(_heads(got, rows, Hq, Hk)) != _bits(want)
    assert not diff.any(), f"{int(diff.sum())} / {diff.numel()} elements differ in bits; first at (row, unit, col) {tuple(int(i) for i in diff.nonzero()[0])}"
    assert torch.equal(_bits(got[:, (Hq + Hk) * 128:]), _bits(buf[:, (Hq + Hk) * 128:])), "v or pad columns changed"


@pytest.mark.parametrize("rows,Hq,Hk", ROPE_SHAPES)
def test_rope_mode1_vs_float64(hip, rows, Hq, Hk):
    """rotate_half = 1, no norm weights: one fp32 expression rounded once, against float64 (bound: module docstring)."""
    buf = _qwen_buffer(rows, Hq, Hk, rows * 11 + Hq)
    cos, sin = _tables(rows, "fp32", rows + Hk + 1)
    x = _heads(buf, rows, Hq, Hk).double()
    pc, ps = x * cos.double()[:, None, :], _rot(x) * sin.double()[:, None, :]
    ref = (pc + ps).bfloat16().double()
    tol = _ulp(ref) + 4 * 2.0 ** -24 * (pc.abs() + ps.abs())
    d = buf.cuda()
    hip.qk_norm_rope(d, Hq, Hk, 0, Hq * 128, cos.cuda(), sin.cuda(), rotate_half=1)
    torch.cuda.synchronize()
    got = d.cpu()
    _check(_heads(got, rows, Hq, Hk), ref, tol, f"rope mode 1 rows={rows} Hq={Hq} Hk={Hk}")
    assert torch.equal(_bits(got[:, (Hq + Hk) * 128:]), _bits(buf[:, (Hq + Hk) * 128:])), "v or pad columns changed"


@pytest.mark.parametrize("mode", [1, 2])
def test_rope_with_norm_weights_and_split(hip, mode):
    """Both half-split modes behind the per-head RMSNorm, (wqA, wkA) for rows < split and (wqB, wkB) after, on the partial-pass shape
    (130 rows, 12 + 2 heads).  float64 reference with the rounding points of csrc/qk_rope_math.h (bound: module docstring)."""
    rows, Hq, Hk, split, eps = 130, 12, 2, 50, 1e-6
    buf = _qwen_buffer(rows, Hq, Hk, 4242 + mode)
    cos, sin = _tables(rows, "bf16" if mode == 2 else "fp32", 99 + mode)
    g = torch.Generator().manual_seed(5 + mode)
    wqA, wkA, wqB, wkB = [(1.0 + 0.3 * torch.randn(128, generator=g) + 0.2 * i).bfloat16() for i in range(4)]
    x = _heads(buf, rows, Hq, Hk).double()
    w = torch.empty(rows, Hq + Hk, 128, dtype=torch.float64)
    w[:split, :Hq], w[:split, Hq:], w[split:, :Hq], w[split:, Hq:] = wqA.double(), wkA.double(), wqB.double(), wkB.double()
    rstd = (1.0 / torch.sqrt((x * x).mean(dim=-1, keepdim=True) + eps)).float().double()
    t = (x * rstd).bfloat16().double()
    n = (t * w).bfloat16().double()
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    if mode == 2:
        ref = ((n * c).bfloat16().double() + (_rot(n) * s).bfloat16().double()).bfloat16().double()
    else:
        ref = (n * c + _rot(n) * s).bfloat16().double()
    e = _ulp(n) + w.abs() * _ulp(t)                                       # what n can be off by, per element
    tol = _ulp(ref) + c.abs() * e + s.abs() * torch.cat((e[..., 64:], e[..., :64]), dim=-1)
    d = buf.cuda()
    hip.qk_norm_rope(d, Hq, Hk, 0, Hq * 128, cos.cuda(), sin.cuda(), split=split, wqA=wqA.cuda(), wkA=wkA.cuda(), wqB=wqB.cuda(),
                     wkB=wkB.cuda(), eps=eps, rotate_half=mode)
    torch.cuda.synchronize()
    got = d.cpu()
    _check(_heads(got, rows, Hq, Hk), ref, tol, f"rope mode {mode} with norm weights, split {split}")
    assert torch.equal(_bits(got[:, (Hq + Hk) * 128:]), _bits(buf[:, (Hq + Hk) * 128:])), "v or pad columns changed"


@pytest.mark.parametrize("mode", [3, -1, 256])
def test_rope_refuses_an_unknown_rotation_mode(hip, mode):
    """rotate_half outside {0, 1, 2}: TD_ERR_INVALID, nothing launched (3 used to run as mode 1)."""
    buf = _qwen_buffer(4, 2, 1, 1)
    cos, sin = _tables(4, "fp32", 2)
    d = buf.cuda()
    with pytest.raises(hip.ThinkDiffHipError, match="error 2"):
        hip.qk_norm_rope(d, 2, 1, 0, 256, cos.cuda(), sin.cuda(), rotate_half=mode)
    torch.cuda.synchronize()
    assert torch.equal(_bits(d.cpu()), _bits(buf))


# ---- td_mrope_table ----------------------------------------------------------------------------------------------------------

MROPE_POS = [0, 1, 63, 64, 1000, 4095, 32767, 131071]


def _streams():
    """int32 [3, 8]: every stream holds every position of MROPE_POS, and t, h, w differ in every column."""
    base = torch.tensor(MROPE_POS, dtype=torch.int32)
    pos = torch.stack([base, torch.roll(base, 1), torch.roll(base, 3)])
    assert ((pos[0] != pos[1]) & (pos[1] != pos[2]) & (pos[0] != pos[2])).all()
    return pos.contiguous()


def _mrope_ref(pos, sections, theta):
    """float64 cos, sin, angle [n, 128]."""
    j = torch.arange(64, dtype=torch.float64)
    inv = torch.tensor(float(theta), dtype=torch.float64) ** (-2.0 * j / 128.0)
    axis = torch.tensor([0] * sections[0] + [1] * sections[1] + [2] * sections[2])
    ang = pos.double()[axis, :].t() * inv[None, :]                     # [n, 64]: column j takes the stream of its section
    ang = torch.cat((ang, ang), dim=1)
    return torch.cos(ang), torch.sin(ang), ang


@pytest.mark.parametrize("round_bf16", [0, 1])
@pytest.mark.parametrize("theta", [1e6, 1e4])
@pytest.mark.parametrize("sections", [(16, 24, 24), (64, 0, 0), (0, 0, 64), (8, 12, 44)])
def test_mrope_table_vs_float64(hip, sections, theta, round_bf16):
    pos = _streams()
    rc, rs, ang = _mrope_ref(pos, sections, theta)
    cos, sin = hip.mrope_table(pos.cuda(), sections, theta, round_bf16)
    torch.cuda.synchronize()
    cos, sin = cos.cpu(), sin.cpu()
    tol = 4 * 2.0 ** -24 * ang.abs() + 4 * 2.0 ** -24
    for name, got, ref in (("cos", cos, rc), ("sin", sin, rs)):
        assert torch.equal(got[:, 64:], got[:, :64]), f"{name}: columns 64 + j differ from columns j"
        if round_bf16:
            assert torch.equal(got.bfloat16().float(), got), f"{name}: values not bf16-representable"
            _check(got, ref, 0.5 * _ulp(ref) + tol, f"mrope {name} sections={sections} theta={theta:g} round_bf16=1")
        else:
            _check(got, ref, tol, f"mrope {name} sections={sections} theta={theta:g} round_bf16=0")


@pytest.mark.parametrize("round_bf16", [0, 1])
def test_mrope_table_structure(hip, round_bf16):
    """Exact properties: with one stream non-zero the other sections' columns are cos = 1, sin = 0 (and its own are not, beyond position
    0); with the three streams equal the sections do not matter."""
    base = torch.tensor(MROPE_POS, dtype=torch.int32)
    sections = (16, 24, 24)
    edges = [0, 16, 40, 64]
    for a in range(3):
        pos = torch.zeros(3, len(MROPE_POS), dtype=torch.int32)
        pos[a] = base
        cos, sin = [t.cpu() for t in hip.mrope_table(pos.cuda(), sections, 1e6, round_bf16)]
        own = torch.zeros(64, dtype=torch.bool)
        own[edges[a]:edges[a + 1]] = True
        assert (cos[:, :64][:, ~own] == 1.0).all() and (sin[:, :64][:, ~own] == 0.0).all(), f"stream {a} leaks into another section"
        assert (sin[1:, :64][:, own] != 0.0).all(), f"stream {a} does not reach its own section"
    pos = torch.stack([base, base, base]).contiguous()
    tabs = [[t.cpu() for t in hip.mrope_table(pos.cuda(), sec, 1e6, round_bf16)] for sec in [(16, 24, 24), (64, 0, 0), (0, 0, 64), (8, 12, 44)]]
    for c, s in tabs[1:]:
        assert torch.equal(c, tabs[0][0]) and torch.equal(s, tabs[0][1])


def test_mrope_table_vs_oracle_bf16(hip):
    """round_bf16 = 1 against oracle.qwen2vl_ref.mrope_cos_sin(..., bfloat16) (torch CPU fp32 arithmetic, cast to bf16) on the streams
    of the tests above plus 248 random columns of positions below 2^17: every element equal or one bf16 ulp apart.  The share that
    differs is printed, not capped.  Measured on MI355X: 0 of 65536 elements differ.

    The regression test of the kernel's inv_freq.  With 1 / powf(theta, j/64) on the device (good to 1 - 2 fp32 ulps, not correctly rounded)
    1852 of the 65536 elements (2.83 %) differed and 572 (0.87 %) by MORE than one bf16 ulp, the nearest at |angle| = 203 rad: beyond
    a few hundred radians one fp32 ulp of the ANGLE is larger than a bf16 ulp of a small cosine, so an inv_freq one ulp off lands several
    bf16 values away.  That kernel still met its float64 bound above -- so does the oracle, whose own tables are more than one bf16 ulp
    from float64 at 836 elements (printed below): at these angles only the same fp32 angle gives the same table.  The kernel now rounds
    theta^(j/64) correctly (through double) and divides in fp32, which is the oracle's inv_freq in all but one column (j = 37 at theta =
    1e6, where torch's 1-ulp pow picks the farther neighbour; its angles stay below 45 rad)."""
    g = torch.Generator().manual_seed(17)
    pos = torch.cat([_streams(), torch.randint(0, 131072, (3, 248), generator=g, dtype=torch.int32)], dim=1).contiguous()
    cfg = Q.Qwen2Config()
    oc, os_ = Q.mrope_cos_sin(pos.long(), cfg, torch.bfloat16)
    rc, rs, ang = _mrope_ref(pos, cfg.mrope_section, cfg.rope_theta)
    cos, sin = hip.mrope_table(pos.cuda(), cfg.mrope_section, cfg.rope_theta, 1)
    torch.cuda.synchronize()
    ndiff = nfar = nfar_oracle = total = 0
    for got, ref, exact in ((cos.cpu().double(), oc.double(), rc), (sin.cpu().double(), os_.double(), rs)):
        ex = exact.bfloat16().double()
        d = (got - ref).abs()
        far = d > torch.maximum(_ulp(got), _ulp(ref))
        ndiff += int((d != 0).sum())
        nfar += int(far.sum())
        nfar_oracle += int(((ref - ex).abs() > torch.maximum(_ulp(ref), _ulp(ex))).sum())
        total += d.numel()
        if far.any():
            print(f"  smallest |angle| of an element more than one ulp apart: {float(ang[far].abs().min()):.0f} rad")
    print(f"mrope round_bf16=1 vs the oracle's bf16 tables: {ndiff} / {total} elements ({100.0 * ndiff / total:.2f} %) differ, {nfar} "
          f"({100.0 * nfar / total:.2f} %) by more than one bf16 ulp; the oracle itself is more than one bf16 ulp from float64 at {nfar_oracle}")
    assert nfar == 0, f"{nfar} / {total} elements more than one bf16 ulp from the oracle"


# ---- td_embed_gather_bf16 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("D", [8, 1536, 2056, 3584])
def test_embed_gather_rows_bit_exact(hip, D, n):
    """out[i] = table[ids[i]] bit for bit: ids include 0, vocab - 1 and repeats; D = 2056 = 257 x 8 takes a second trip of the 256-thread
    copy loop.  The rows of out past n (the buffer is longer) stay untouched."""
    vocab = 77
    g = torch.Generator().manual_seed(D + n)
    table = torch.randn(vocab, D, generator=g).bfloat16()
    ids = torch.randint(0, vocab, (n,), generator=g, dtype=torch.int32)
    ids[0] = vocab - 1
    if n > 1:
        ids[1], ids[2], ids[3], ids[n - 1] = 0, vocab - 1, 5, 5
    buf = torch.full((n + 2, D), -7.0, dtype=torch.bfloat16, device="cuda")
    hip.embed_gather(ids.cuda(), table.cuda(), out=buf[:n])
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(_bits(got[:n]), _bits(table[ids.long()]))
    assert (got[n:].float() == -7.0).all(), "rows past n written"


def test_embed_gather_clamps_out_of_range_ids(hip):
    """The documented clamp (include/thinkdiff_hip.h): id < 0 reads row 0, id >= vocab reads row vocab - 1; the table sits inside a
    larger buffer whose neighbouring rows hold a sentinel that must not come back."""
    vocab, D = 50, 1536
    g = torch.Generator().manual_seed(1)
    big = torch.full((vocab + 2, D), 1e4).bfloat16()
    big[1:vocab + 1] = torch.randn(vocab, D, generator=g).bfloat16()
    table = big[1:vocab + 1]
    ids = torch.tensor([-1, vocab, 2 ** 31 - 1, -2 ** 31, 0, vocab - 1, 7], dtype=torch.int32)
    want = table[[0, vocab - 1, vocab - 1, 0, 0, vocab - 1, 7]]
    out = hip.embed_gather(ids.cuda(), big.cuda()[1:vocab + 1])
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.cpu()), _bits(want))
