"""Context attention (td_attention_prefix_segments_bf16: packed causal query segments over key ranges of their own in a cache-shaped buffer,
td_attn_fwd_d128_lean_kernel<true, 8, false, true, false, true, false, true>) against float64, on operands whose decisiveness
tests/test_attention_prefix_cases_cpu.py asserts: a causal offset one off, a dropped first key or prefix, a neighbouring slot's rows, another segment's
kv_seg_row0 or an offset taken from the longest segment each miss the bar used here by >= 81x (tests/attention_prefix_cases_common.py).

Bar: |err| <= 2^-7 max|ref| per segment, the bar of tests/test_attention_packed_gpu.py.  The comparisons with the existing launches are held within the
same bar; what was measured of bit equality is stated in the tests' docstrings.

Measured on MI355X, worst ratio to the bar: 0.46 at (Hq, Hkv) = (4, 2) (segment (1, 1)) and 0.47 at (7, 1) (segment (255, 1)); 0.19 .. 0.47 over all
segments with more than one key.
"""
import pytest
import torch

import attention_cases_common as C
import attention_prefix_cases_common as P

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
OUT_PAD = 40


def _launch(hip, case, dq, dcache, max_q, max_kv):
    """One launch on the case's buffers -> out [R, Hq*128 + OUT_PAD], pre-filled with the sentinel."""
    Hq, Hkv = case["Hq"], case["Hkv"]
    KW = Hkv * P.D
    wide = torch.full((case["R"], Hq * P.D + OUT_PAD), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hip.attention_prefix_segments(dq[:, :Hq * P.D], dcache[:, :KW], dcache[:, KW:2 * KW], wide[:, :Hq * P.D], Hq, Hkv, case["starts"].cuda(), case["row0"].cuda(),
                                  case["kv_lens"].cuda(), max_q, max_kv, P.SCALE)
    return wide


def _ratios(got, ref, starts):
    return [float((got[starts[s]:starts[s + 1]] - ref[starts[s]:starts[s + 1]]).abs().max() / (P.BAR * ref[starts[s]:starts[s + 1]].abs().max()))
            for s in range(len(starts) - 1)]


@pytest.mark.parametrize("Hq,Hkv", P.HEADS)
def test_prefix_segments_against_float64(hip, Hq, Hkv):
    """One launch over the 15 (q_len, prefix) segments, k / v in a cache of 1400-row slots taken in scrambled order, every row outside a segment's keys
    holding 1e4, q and out inside wider rows.  Per segment |err| <= 2^-7 max|ref| against float64; the pad columns of out keep the sentinel; a second
    launch gives the same bits; max_q_len and max_kv_len beyond the longest (more query-tile columns of workgroups, which must all leave; a larger
    range check) give the same bits."""
    case = P.prefix_case(Hq, Hkv)
    dq, dcache = case["qbuf"].cuda(), case["cache"].cuda()
    mq, mkv = max(case["q_lens"]), int(case["kv_lens"].max())
    outs = [_launch(hip, case, dq, dcache, mq, mkv), _launch(hip, case, dq, dcache, mq, mkv), _launch(hip, case, dq, dcache, mq + 300, mkv + 1000)]
    torch.cuda.synchronize()
    wide = outs[0]
    assert (wide[:, Hq * P.D:].float() == SENTINEL).all(), "pad columns of out written"
    got = wide[:, :Hq * P.D].double().cpu()
    assert torch.isfinite(got).all()
    ratios = _ratios(got, case["ref"], case["starts"].tolist())
    at = max(range(len(ratios)), key=ratios.__getitem__)
    print(f"prefix segments Hq={Hq} Hkv={Hkv}: max error {ratios[at]:.3f} x the bar (segment {at} {P.CASES[at]}); per segment " + " ".join(f"{r:.2f}" for r in ratios))
    assert ratios[at] <= 1.0, f"segment {at} {P.CASES[at]}: max error {ratios[at]:.3f} x the bar"
    assert torch.equal(outs[0], outs[1]), "a repeated launch gave different bits"
    assert torch.equal(outs[0], outs[2]), "max_q_len / max_kv_len beyond the longest changed the bits"


@pytest.mark.parametrize("Hq,Hkv", P.HEADS)
def test_prefix_segments_against_each_segment_alone(hip, Hq, Hkv):
    """Each segment alone through hip.attention(causal=True) on its own [kv_len] rows (td_attention_bf16 with Sq <= Skv: the unpacked causal instantiation
    of the tile kernel, the decode kernel for the one-row segments) agrees with its rows of the packed launch within the bar.  Measured on MI355X, both
    head configurations: 12 of 15 segments bit-equal; the three that are not are the one-row segments with a prefix, (1, 1), (1, 63) and (1, 64), which the
    unpacked launch hands to the decode kernel (another summation order).  So equality is asserted for every segment the tile kernel runs either way, and
    for (1, 0), whose one key makes the row its value row under any kernel."""
    case = P.prefix_case(Hq, Hkv)
    dq, dcache = case["qbuf"].cuda(), case["cache"].cuda()
    KW = Hkv * P.D
    packed = _launch(hip, case, dq, dcache, max(case["q_lens"]), int(case["kv_lens"].max()))[:, :Hq * P.D]
    starts = case["starts"].tolist()
    equal = []
    for b, (n, p) in enumerate(P.CASES):
        a, r0 = starts[b], int(case["row0"][b])
        alone = torch.full((1, n, Hq * P.D), SENTINEL, dtype=torch.bfloat16, device="cuda")
        hip.attention(dq[None, a:a + n, :Hq * P.D], dcache[None, r0:r0 + n + p, :KW], dcache[None, r0:r0 + n + p, KW:2 * KW], alone, Hq, Hkv, P.SCALE, causal=True)
        torch.cuda.synchronize()
        d = float((packed[a:a + n].double() - alone[0].double()).abs().max())
        assert d <= P.BAR * float(alone.double().abs().max()), f"segment {b} {(n, p)} differs from the segment run alone by {d:.3g}"
        equal.append(bool(torch.equal(packed[a:a + n], alone[0])))
    print(f"prefix segments Hq={Hq} Hkv={Hkv}: bit-equal to the single-segment launch: {sum(equal)} of {len(equal)} "
          f"(not equal: {[P.CASES[b] for b, e in enumerate(equal) if not e]})")
    assert all(e for e, (n, p) in zip(equal, P.CASES) if n > 1 or p == 0)


@pytest.mark.parametrize("Hq,Hkv", C.PACKED_HEADS)
def test_prefix_zero_is_the_packed_causal_launch(hip, Hq, Hkv):
    """Every prefix 0 and k / v the packed rows themselves (kv_row0 = seg_starts, kv_lens = the segments' lengths), on the operands of
    tests/test_attention_packed_gpu.py: the output of attention_segments(causal=True) within the bar, and within the bar of float64.  Measured on
    MI355X: all 13 segments of both head configurations bit-equal to the packed causal launch (the form only moves the K / V base pointers and takes
    Skv and the causal offset, 0 here, from the arrays), so equality is asserted."""
    case = C.packed_case(Hq, Hkv)
    dbuf = case["buf"].cuda()
    S = case["S"]
    q0, k0, v0 = case["cols"]
    q, k, v = dbuf[:S, q0:q0 + Hq * C.D], dbuf[:S, k0:k0 + Hkv * C.D], dbuf[:S, v0:v0 + Hkv * C.D]
    starts = case["starts"].cuda()
    lens = torch.tensor(case["lens"], dtype=torch.int32).cuda()
    want = torch.full((S, Hq * C.D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    got = torch.full((S, Hq * C.D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hip.attention_segments(q, k, v, want, Hq, Hkv, starts, max(case["lens"]), C.SCALE, True)
    hip.attention_prefix_segments(q, k, v, got, Hq, Hkv, starts, starts[:-1].contiguous(), lens, max(case["lens"]), max(case["lens"]), C.SCALE)
    torch.cuda.synchronize()
    st = case["starts"].tolist()
    r = _ratios(got.double().cpu(), want.double().cpu(), st)
    r64 = _ratios(got.double().cpu(), case["ref"], st)
    eq = [bool(torch.equal(got[st[s]:st[s + 1]], want[st[s]:st[s + 1]])) for s in range(len(st) - 1)]
    print(f"prefix 0 Hq={Hq} Hkv={Hkv}: against the packed causal launch {max(r):.3f} x the bar, against float64 {max(r64):.3f} x the bar, "
          f"bit-equal segments {sum(eq)} of {len(eq)}")
    assert max(r) <= 1.0 and max(r64) <= 1.0
    assert all(eq)


def test_launcher_refusals_name_the_form(hip):
    """The C entry refuses what the form does not serve before anything is launched."""
    L = hip.lib()
    z = torch.zeros(4, 128, dtype=torch.bfloat16, device="cuda")
    i = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = hip.ptr
    assert L.td_attention_prefix_segments_bf16(p(z), p(z), p(z), p(z), 128, 128, 128, p(i), None, p(i), 1, 1, 1, 1, 1, 0.1, None) == 2
    assert b"kv_row0 and kv_lens are both required" in L.td_last_error()
    assert L.td_attention_prefix_segments_bf16(p(z), p(z), p(z), p(z), 128, 128, 128, p(i), p(i), p(i), 1, 4, 2, 1, 1, 0.1, None) == 2
    assert b"max_kv_len=2 is below max_q_len=4" in L.td_last_error()
