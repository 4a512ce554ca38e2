"""The VAE's implicit-GEMM 3x3 convolutions (td_conv3x3_nhwc_bf16, td_conv3x3_s2_nhwc_bf16: csrc/gemm_bf16.hip gemm_tile with CONV = 1 / 2)
against float64, element by element, on the cases of tests/vae_conv_common.py -- every element of every case is compared, none is sampled.

Three comparisons per case (the makers of vae_conv_common): integer operands, where every partial sum is exact and the kernel must return the
float64 reference's bf16 value bit for bit; the one-hot weight, whose expected output is written down by indexing the input; random operands
under the derived per-element bound `tol` (one bf16 ulp per rounding point of the tile epilogue + K 2^-24 sum |x||w|; the bound is derived in
vae_conv_common's docstring and set by nothing measured).  tests/test_vae_conv_cases_cpu.py shows that each comparison rejects a kernel whose
border taps wrap or clamp, that pads the wrong side, takes the upsample's parent before the tap, drops a channel run, reads the weights in
torch's order or lets rows past M alias pixel 0.

Which instantiation a case runs is td_gemm_launch's routing on N = Cout (`instantiation`): <= 64 launch_cfg<8, 1, CONV>, <= 128
launch_cfg<8, 2, CONV>, else launch_cfg<8, 4, CONV>, CONV = 2 for the stride-2 form.  The one-hot runs have Cout = 72: launch_cfg<8, 2, CONV>
with a ragged n.  Output buffers are exactly [M, Cout]: a store past N or M would land in somebody else's memory, not in padding.

Measured on MI355X, worst error / bound per random case: profiles/vae_conv_fp64_bounds.json (written by the random test; a record only).
"""
import pytest
import torch

import vae_conv_common as C

pytestmark = pytest.mark.gpu

IDS = [C.case_id(c) for c in C.CASES]


def _run(hip, form, x, w, bias, res=None, alias=False, Cout_pad=None, Cin_pad=None):
    """The HIP convolution of x [Hin, Win, Cin] (CPU bf16) -> float64 [M, Cout_pad or Cout] on the CPU.  alias: the residual buffer is the output."""
    H, W = C.out_extent(form, x)
    Cout = Cout_pad or w.shape[0]
    xin = x.reshape(-1, x.shape[-1]).contiguous().cuda()
    wp = hip.conv3x3_pack_weight(w.cuda(), Cout_pad=Cout_pad, Cin_pad=Cin_pad)
    assert wp.shape == (Cout, 9 * xin.shape[1])
    b = None if bias is None else bias.cuda()
    if form == "s2":
        assert res is None
        y = hip.conv3x3_s2_nhwc(xin, wp, b, H, W, Cout)
    else:
        r = None if res is None else res.cuda()
        y = hip.conv3x3_nhwc(xin, wp, b, H, W, Cout, res=r, upsample2x=form == "up", out=r if alias else None)
    torch.cuda.synchronize()
    _, _, Ho, Wo = C.extents(form, H, W)
    assert y.shape == (Ho * Wo, Cout) and y.dtype == torch.bfloat16
    return y.cpu()


def _aliased_is_bit_equal(hip, form, R, y):
    """The residual may be the output buffer (vae_common.h's resnet adds its input in place): the same bits."""
    if R["res"] is not None:
        ya = _run(hip, form, R["x"], R["w"], R["bias"], R["res"], alias=True)
        assert torch.equal(ya.view(torch.int16), y.view(torch.int16)), "residual aliasing the output changes the result"


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_conv3x3_integer_bit_exact(hip, case):
    form = case[0]
    R = C.reference(case, "integer")
    assert C.integer_condition(R["dot"], R["bias"], R["res"]) <= 256
    y = _run(hip, form, R["x"], R["w"], R["bias"], R["res"])
    C.check_exact(y, R["want"], f"{C.case_id(case)} [{C.instantiation(case)}] integer")      # (equal bf16 values are equal bits, but for a zero's sign)
    _aliased_is_bit_equal(hip, form, R, y)


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_conv3x3_one_hot_copies_the_tap(hip, case):
    form = case[0]
    x, w = C.make_one_hot(case)
    y = _run(hip, form, x, w, None)
    C.check_exact(y, C.hot_expected(form, x), f"{C.case_id(case)} [launch_cfg<8, 2, {'2' if form == 's2' else 'true'}>, Cout 72] one-hot")


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_conv3x3_random_within_derived_bound(hip, case):
    form = case[0]
    R = C.reference(case, "random")
    y = _run(hip, form, R["x"], R["w"], R["bias"], R["res"])
    worst = C.check_tol(y, R["cmp"], R["tol"], f"{C.case_id(case)} [{C.instantiation(case)}] random")
    C.record(C.case_id(case), worst)
    _aliased_is_bit_equal(hip, form, R, y)


# ---- the decoder's ends as the engine runs them -----------------------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("maker", ["integer", "random"])
def test_conv_in_padded_input_channels(hip, maker):
    """Decoder.conv_in: 16 latent channels in a 64-channel NHWC buffer, the weight packed with Cin_pad = 64.  The buffer's channels >= 16 hold a
    non-zero sentinel: the packed weight's pad columns must be zero, or the sentinel shows.  (No one-hot run: its channel rule needs Cin >= 64.)
    K = 576 is what the kernel sums; 360 of the products are sentinel x 0, exact zeros."""
    H, W, Cin, Cpad, Cout = 6, 10, 16, 64, 512
    g = _gen(11 if maker == "integer" else 12)
    if maker == "integer":
        tri = lambda *s: (torch.randint(0, 2, s, generator=g) * (2 * torch.randint(0, 2, s, generator=g) - 1)).bfloat16()
        x, w, bias, sentinel = tri(H, W, Cin), tri(Cout, Cin, 3, 3), torch.randint(-4, 5, (Cout,), generator=g).bfloat16(), 7.0
    else:
        x = torch.randn(H, W, Cin, generator=g).bfloat16()
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).bfloat16()
        bias, sentinel = torch.randn(Cout, generator=g).bfloat16(), 3.0
    xp = torch.full((H, W, Cpad), sentinel, dtype=torch.bfloat16)
    xp[..., :Cin] = x
    y = _run(hip, "s1", xp, w, bias, Cin_pad=Cpad)
    dot, absdot = C.ref("s1", x, w)
    cmp, want = C.expected(dot, bias, None)
    if maker == "integer":
        assert C.integer_condition(dot, bias, None) <= 256
        C.check_exact(y, want, "conv_in integer")
    else:
        C.record("conv_in-6x10-16(64)to512", C.check_tol(y, cmp, C.tol(dot, absdot, bias, None, 9 * Cpad), "conv_in random"))


@pytest.mark.parametrize("maker", ["integer", "one_hot", "random"])
def test_conv_out_padded_output_channels(hip, maker):
    """Decoder.conv_out: 128 -> 3 channels, packed to Cout_pad = 8 rows.  Columns 0 .. 2 are the convolution; columns 3 .. 7 have all-zero
    weight rows and must equal their bias pad exactly (a non-zero pad here, so that a dropped or misplaced column shows)."""
    H, W, Cin, Cout, Cpad = 7, 9, 128, 3, 8
    case = ("s1", H, W, Cin, Cout, False)
    pad = torch.tensor([0.5, -1.25, 3.0, -7.0, 100.0]).bfloat16()
    if maker == "one_hot":
        x, w = C.make_one_hot(case, Cout_hot=Cout)
        bias = torch.zeros(Cout).bfloat16()
    else:
        x, w, bias, _ = (C.make_integer if maker == "integer" else C.make_random)(case)
    y = _run(hip, "s1", x, w, torch.cat([bias, pad]), Cout_pad=Cpad)
    assert torch.equal(y[:, Cout:].double(), pad.double().expand(H * W, Cpad - Cout)), "pad columns differ from the bias pad"
    got = y[:, :Cout]
    if maker == "one_hot":
        C.check_exact(got, C.hot_expected("s1", x, Cout_hot=Cout), "conv_out one-hot")
        return
    dot, absdot = C.ref("s1", x, w)
    cmp, want = C.expected(dot, bias, None)
    if maker == "integer":
        assert C.integer_condition(dot, bias, None) <= 256
        C.check_exact(got, want, "conv_out integer")
    else:
        C.record("conv_out-7x9-128to3(8)", C.check_tol(got, cmp, C.tol(dot, absdot, bias, None, 9 * Cin), "conv_out random"))


@pytest.mark.parametrize("Cout,Cin,Cout_pad,Cin_pad", [(8, 64, 8, 64), (3, 128, 8, 128), (128, 16, 128, 64), (5, 3, 8, 64)])
def test_conv3x3_pack_weight_bit_exact(hip, Cout, Cin, Cout_pad, Cin_pad):
    """td_conv3x3_pack_weight against a torch permute + zero pad, bit for bit (-0.0 and the pad's +0.0 included)."""
    w = torch.randn(Cout, Cin, 3, 3, generator=_gen(Cout * 131 + Cin)).bfloat16()
    w.view(-1)[:3] = torch.tensor([-0.0, 0.0, 3.3895e38]).bfloat16()
    got = hip.conv3x3_pack_weight(w.cuda(), Cout_pad=Cout_pad, Cin_pad=Cin_pad)
    torch.cuda.synchronize()
    want = C.pack(w, Cout_pad, Cin_pad)
    assert got.shape == want.shape == (Cout_pad, 9 * Cin_pad)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
