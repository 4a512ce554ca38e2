"""The cases of tests/vae_conv_common.py can see what they are for: every deliberately wrong convolution of WRONG, given the case's own operands
and rounded to bf16 as the kernel rounds, is rejected by each of the three comparisons that tests/test_vae_conv_fp64_gpu.py makes of the HIP
kernel.  No GPU: the "kernel" here is a float64 im2col product with one fault.

What rejects what (every case of CASES on which the fault changes what is read at all; `applies` says where it does not):

  variant            integer (bit for bit)   one-hot (by value)      random (under tol)     does not apply to
  wrap               every case              every case              every case             --
  clamp              every case              every case              every case             --
  pad_top_left       every s2 case           every s2 case           every s2 case          s1, up (there is no such pad)
  parent_before_tap  every up case           every up case           every up case          s1, s2 (there is no parent)
  drop_last_chunk    every case it applies   every case it applies   every case it applies  s1 1x7, 7x1, 1x257 and s2 2x2, 2x10, 10x2: tap 8
                                                                                            (dy = dx = +1) is inside the image for no pixel
  k_order            every case              every case              every case             --
  rows_past_m        every case it applies   every case it applies   every case it applies  s2 2x2 (one output pixel: the last pixel IS pixel 0)

`drop_last_chunk` and the one-hot weight: output channel o = 9 j + 8 reads tap 8 of input channel j (Cin / 8) + 3, and for every Cin of CASES
(64, 128, 192, 256, 512) at least the j = 7 channel lies in the last 64 -- asserted below -- so the one-hot comparison covers the dropped run on
every case the fault applies to.

Findings about the random bound's power: none.  Under `tol` the random comparison rejects every variant on every case it applies to; the
smallest fault, `drop_last_chunk` at Cin = 512 (64 of 4608 products), still moves border-free pixels by about 0.12 against a bound of about 2^-7.
Every assertion below is unconditional: a variant that slipped through any of the three comparisons fails this file.
"""
import pytest
import torch

import vae_conv_common as C

IDS = [C.case_id(c) for c in C.CASES]


def _variants(case):
    form, H, W = case[:3]
    return [name for name in C.WRONG if C.applies(name, form, H, W)]


def test_cases_cover_the_forms_and_tiles():
    """The six instantiations launch_cfg<8, {1, 2, 4}, {true, 2}> each run at least one case, and every variant of WRONG applies somewhere."""
    assert {C.instantiation(c) for c in C.CASES} == {f"launch_cfg<8, {wn}, {cv}>" for wn in (1, 2, 4) for cv in ("true", "2")}
    for name in C.WRONG:
        assert any(name in _variants(c) for c in C.CASES), name
    # where a fault does not apply, its index map is the right one (or its form has no such step): the list of the module docstring
    skipped = {(C.case_id(c), n) for c in C.CASES for n in C.WRONG if c[0] in C.WRONG_FORMS[n] and n not in _variants(c)}
    assert skipped == {(i, "drop_last_chunk") for i in ("s1-1x7-64to8", "s1-7x1-64to64", "s1-1x257-64to64", "s2-2x2-64to64", "s2-2x10-64to8",
                                                         "s2-10x2-64to32")} | {("s2-2x2-64to64", "rows_past_m")}


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_reference_agrees_with_indexing(case):
    """float64 F.conv2d gives, for the one-hot weight, exactly what indexing the input gives: two statements of the geometry, one answer."""
    form = case[0]
    x, w = C.make_one_hot(case)
    hot = C.hot_expected(form, x)
    dot, absdot = C.ref(form, x, w)
    assert dot.shape == hot.shape == (C.extents(*case[:3])[2] * C.extents(*case[:3])[3], C.COUT_HOT)
    assert torch.equal(dot, hot) and torch.equal(absdot, hot.abs())
    assert bool((hot == 0).any()) and bool((hot != 0).any())      # some taps are outside the image, some inside


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_integer_condition(case):
    R = C.reference(case, "integer")
    m = C.integer_condition(R["dot"], R["bias"], R["res"])
    print(f"{C.case_id(case)}: largest |partial result| {m:.0f}")
    assert m <= 256
    assert torch.equal(R["cmp"], R["want"])                        # nothing is rounded away: the reference is its own bf16 value
    assert torch.equal(R["dot"], R["dot"].round())


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_integer_comparison_rejects_every_wrong_convolution(case):
    form = case[0]
    R = C.reference(case, "integer")
    C.check_exact(R["want"], R["want"], "the reference itself")
    for name in _variants(case):
        got = C.expected(C.WRONG[name](form, R["x"], R["w"], R["bias"])[0], R["bias"], R["res"])[1]
        with pytest.raises(AssertionError, match="elements differ"):
            C.check_exact(got, R["want"], name)


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_one_hot_comparison_rejects_every_wrong_convolution(case):
    form, _, _, Cin = case[:4]
    x, w = C.make_one_hot(case)
    hot = C.hot_expected(form, x)
    # drop_last_chunk reaches a hot channel: o = 9 j + 8 reads tap 8 of channel j (Cin / 8) + 3
    assert any(o % 9 == 8 and (o // 9) * (Cin // 8) + 3 >= Cin - 64 for o in range(C.COUT_HOT))
    for name in _variants(case):
        got = C.bf(C.WRONG[name](form, x, w)[0])
        with pytest.raises(AssertionError, match="elements differ"):
            C.check_exact(got, hot, name)


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_random_comparison_rejects_every_wrong_convolution(case):
    form = case[0]
    R = C.reference(case, "random")
    assert C.check_tol(R["want"], R["cmp"], R["tol"], "the reference's own rounding") <= 0.5 + 1e-9      # half an ulp of the one ulp allowed
    for name in _variants(case):
        got = C.expected(C.WRONG[name](form, R["x"], R["w"], R["bias"])[0], R["bias"], R["res"])[1]
        with pytest.raises(AssertionError, match="beyond the bound"):
            C.check_tol(got, R["cmp"], R["tol"], name)


def test_pack_is_a_permute_and_a_pad():
    w = torch.arange(2 * 3 * 9, dtype=torch.float32).reshape(2, 3, 3, 3).bfloat16()
    p = C.pack(w, Cout_pad=4, Cin_pad=5).view(4, 9, 5)
    for o in range(4):
        for t in range(9):
            for c in range(5):
                want = float(w[o, c, t // 3, t % 3]) if o < 2 and c < 3 else 0.0
                assert float(p[o, t, c]) == want
