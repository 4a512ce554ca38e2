"""Packed causal attention (td_attention_segments_bf16, causal = 1: the launch of the Qwen2-VL engine's packed prefill,
td_attn_fwd_d128_lean_kernel<true, 8, false, true>) and cached prefill (td_attention_bf16, causal, 1 < Sq < Skv) against float64, on
operands whose decisiveness tests/test_attention_cases_cpu.py asserts: every masking / indexing mutant of the reference lies >= 10x the bar
used here from the true one (tests/attention_cases_common.py).

Bar: the module bar of tests/test_attention_gpu.py, |err| <= 2^-7 max|ref| (P is rounded to bf16 in front of the PV product, the output is
bf16), the maximum taken per segment (packed) or per batch entry (cached prefill).

Measured on MI355X, worst ratio to the bar: packed causal 0.46 at (Hq, Hkv) = (4, 2) and 0.38 at (7, 1); cached prefill 0.26 .. 0.37 over the five
shapes and both batch entries, the same under all three kernel variants; every packed segment bit-equal to the same segment launched alone.
"""
import pytest
import torch

import attention_cases_common as C

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
OUT_PAD = 40          # ldo = Hq * 128 + 40 > Hq * 128


def _launch(hip, case, dbuf, max_len, causal=True):
    """One td_attention_segments_bf16 launch on the case's buffer -> out [S, Hq*128 + OUT_PAD], pre-filled with the sentinel."""
    Hq, Hkv, S = case["Hq"], case["Hkv"], case["S"]
    q0, k0, v0 = case["cols"]
    wide = torch.full((S, Hq * C.D + OUT_PAD), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hip.attention_segments(dbuf[:S, q0:q0 + Hq * C.D], dbuf[:S, k0:k0 + Hkv * C.D], dbuf[:S, v0:v0 + Hkv * C.D], wide[:, :Hq * C.D], Hq, Hkv,
                           case["starts"].cuda(), max_len, C.SCALE, causal)
    return wide


def _worst_per_segment(got, ref, starts):
    """max over segments of max|got - ref| / (2^-7 max|ref|), each maximum inside the segment; and the segment it is reached in."""
    worst, at = 0.0, -1
    for s in range(len(starts) - 1):
        a, b = starts[s], starts[s + 1]
        r = float((got[a:b] - ref[a:b]).abs().max() / (C.BAR * ref[a:b].abs().max()))
        if r > worst:
            worst, at = r, s
    return worst, at


@pytest.mark.parametrize("Hq,Hkv", C.PACKED_HEADS)
def test_packed_causal_segments_against_float64(hip, Hq, Hkv):
    """One launch over segments of 1, 2, 31, 32, 33, 64, 65, 255, 256, 257, 300, 513 and 1 rows, q | k | v inside wider rows whose pad columns hold
    1e4, out inside wider rows pre-filled with a sentinel.  Per segment |err| <= 2^-7 max|ref| against float64; the pad columns of out keep
    the sentinel; a second launch gives the same bits; a launch with max_len larger than the longest segment (a fourth query-tile column
    of workgroups that must all leave) gives the same bits."""
    case = C.packed_case(Hq, Hkv)
    dbuf = case["buf"].cuda()
    longest = max(case["lens"])
    outs = [_launch(hip, case, dbuf, longest), _launch(hip, case, dbuf, longest), _launch(hip, case, dbuf, longest + 300)]
    torch.cuda.synchronize()
    wide = outs[0]
    assert (wide[:, Hq * C.D:].float() == SENTINEL).all(), "pad columns of out written"
    got = wide[:, :Hq * C.D].double().cpu()
    assert torch.isfinite(got).all()
    worst, at = _worst_per_segment(got, case["ref"], case["starts"].tolist())
    print(f"packed causal Hq={Hq} Hkv={Hkv}: max error {worst:.3f} x the bar (segment {at}, {case['lens'][at]} rows)")
    assert worst <= 1.0, f"segment {at} ({case['lens'][at]} rows): max error {worst:.3f} x the bar"
    assert torch.equal(outs[0], outs[1]), "a repeated launch gave different bits"
    assert torch.equal(outs[0], outs[2]), "max_len beyond the longest segment changed the bits"


@pytest.mark.parametrize("Hq,Hkv", C.PACKED_HEADS)
def test_packed_segments_equal_each_segment_alone(hip, Hq, Hkv):
    """Each segment run alone through hip.attention(causal=True) (td_attention_bf16: the unpacked causal instantiation of the same tile
    kernel; the dedicated decode kernel for the one-row segments) agrees with its rows of the packed launch within the bar -- and bit for bit:
    measured on MI355X, all 13 segments of both head configurations are bit-equal to the single-segment launch (the packed form only moves the
    operand base pointers and takes Sq = Skv from seg_starts; a one-row segment is its value row under either kernel), so equality is asserted."""
    case = C.packed_case(Hq, Hkv)
    dbuf = case["buf"].cuda()
    q0, k0, v0 = case["cols"]
    packed = _launch(hip, case, dbuf, max(case["lens"]))[:, :Hq * C.D]
    starts = case["starts"].tolist()
    equal = []
    for s, n in enumerate(case["lens"]):
        a, b = starts[s], starts[s + 1]
        alone = torch.full((1, n, Hq * C.D), SENTINEL, dtype=torch.bfloat16, device="cuda")
        hip.attention(dbuf[None, a:b, q0:q0 + Hq * C.D], dbuf[None, a:b, k0:k0 + Hkv * C.D], dbuf[None, a:b, v0:v0 + Hkv * C.D], alone, Hq, Hkv, C.SCALE, causal=True)
        torch.cuda.synchronize()
        d = (packed[a:b].double() - alone[0].double()).abs().max()
        assert float(d) <= C.BAR * float(alone.double().abs().max()), f"segment {s} ({n} rows) differs from the segment run alone by {float(d):.3g}"
        equal.append(bool(torch.equal(packed[a:b], alone[0])))
    print(f"packed causal Hq={Hq} Hkv={Hkv}: segments bit-equal to the single-segment launch: {sum(equal)} of {len(equal)} "
          f"(not equal: {[case['lens'][s] for s, e in enumerate(equal) if not e]} rows)")
    assert all(equal)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("Hq,Hkv", C.PACKED_HEADS)
def test_packed_one_row_segments_only(hip, Hq, Hkv, causal):
    """max_len = 1: five segments of one row each (a prefill pass of one-token prompts).  A causal launch with Sq = Skv = 1 has the shape of a
    decode step, and td_attn_launch used to hand it to the decode kernel, which knows no seg_starts and steps by the batch strides (0 in a packed
    launch): every segment read row 0 and wrote row 0, rows 1 .. 4 of out kept the sentinel.  Packed launches now stay on the tile kernel.
    float64 reference: softmax over one key is 1, so every output row is the value row of its kv head -- within the bar, and in fact exactly
    (v . p / p with one bf16 p differs from v by fp32 rounding only).  Measured on MI355X: 305 .. 513 x the bar on segments 1 .. 4 before the
    fix (causal; the full form never took that route), 0 after."""
    n = 5
    g = torch.Generator().manual_seed(Hq * 10 + Hkv)
    ld = (Hq + 2 * Hkv) * C.D + 24
    buf = torch.randn(n, ld, generator=g).bfloat16()
    dbuf = buf.cuda()
    q0, k0, v0 = 0, Hq * C.D + 8, Hq * C.D + 8 + Hkv * C.D + 8
    starts = torch.arange(n + 1, dtype=torch.int32).cuda()
    wide = torch.full((n, Hq * C.D + OUT_PAD), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hip.attention_segments(dbuf[:, q0:q0 + Hq * C.D], dbuf[:, k0:k0 + Hkv * C.D], dbuf[:, v0:v0 + Hkv * C.D], wide[:, :Hq * C.D], Hq, Hkv, starts, 1, C.SCALE, causal)
    torch.cuda.synchronize()
    ref = buf[:, v0:v0 + Hkv * C.D].double().reshape(n, Hkv, 1, C.D).expand(n, Hkv, Hq // Hkv, C.D).reshape(n, Hq * C.D)
    got = wide[:, :Hq * C.D].double().cpu()
    assert (wide[:, Hq * C.D:].float() == SENTINEL).all(), "pad columns of out written"
    ratios = [float((got[s] - ref[s]).abs().max() / (C.BAR * ref[s].abs().max())) for s in range(n)]
    print(f"one-row segments Hq={Hq} Hkv={Hkv} causal={causal}: max error " + ", ".join(f"{r:.3f}" for r in ratios) + " x the bar per segment")
    assert max(ratios) <= 1.0, f"one-row segments: max error {max(ratios):.3f} x the bar"
    assert torch.equal(got, ref), "a one-row segment is not its own value row"


def test_segments_entry_without_causal_is_the_varlen_entry(hip):
    """causal = 0: the bits of td_attention_varlen_bf16 on the same operands (one fused [S, 3 H 128] buffer, the vision towers' layout)."""
    H, lens = 2, [300, 1, 64, 257, 31]
    S = sum(lens)
    g = torch.Generator().manual_seed(17)
    qkv = torch.randn(S, 3 * H * C.D, generator=g).bfloat16().cuda()
    starts = torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32).cuda()
    want = hip.attention_padded_varlen(qkv, H, C.SCALE, starts, max(lens))
    W = H * C.D
    got = torch.full((S, W), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hip.attention_segments(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], got, H, H, starts, max(lens), C.SCALE, causal=False)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.fixture(params=[0, 1, 2], ids=["auto", "one_wg_per_item", "streamk_no_remap"])
def variant(request, hip):
    """The three kernel variants of tests/test_attention_gpu.py's autouse fixture."""
    prev = hip.lib().td_attention_set_variant(request.param)
    yield request.param
    hip.lib().td_attention_set_variant(prev)


@pytest.mark.parametrize("Sq,Skv", C.PREFILL_SHAPES)
def test_cached_prefill_planted_keys(hip, variant, Sq, Skv):
    """1 < Sq < Skv, causal, batch 2, (Hq, Hkv) = (12, 2), k / v from a cache-shaped buffer whose rows past Skv hold 1e4, with successor and
    diagonal keys planted at query rows 0, 31, 32, Sq - 2, Sq - 1 and key 0 made dominant for the last row: causal_offset +- 1 or a dropped
    first key would miss the bar by >= 115x (tests/test_attention_cases_cpu.py).  |err| <= 2^-7 max|ref| per batch entry against float64."""
    case = C.prefill_case(Sq, Skv)
    Hq, Hkv = C.PREFILL_HQ, C.PREFILL_HKV
    dbuf = case["buf"].cuda()
    out = torch.full((C.PREFILL_B, Sq, Hq * C.D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hip.attention(case["q"].cuda(), dbuf[:, :Skv, :Hkv * C.D], dbuf[:, :Skv, Hkv * C.D:2 * Hkv * C.D], out, Hq, Hkv, causal=True)
    torch.cuda.synchronize()
    got, ref = out.double().cpu(), case["ref"]
    assert torch.isfinite(got).all()
    ratios = [float((got[b] - ref[b]).abs().max() / (C.BAR * ref[b].abs().max())) for b in range(C.PREFILL_B)]
    print(f"cached prefill ({Sq}, {Skv}) variant {variant}: max error " + ", ".join(f"{r:.3f}" for r in ratios) + " x the bar per batch entry")
    assert max(ratios) <= 1.0, f"max error {max(ratios):.3f} x the bar"
