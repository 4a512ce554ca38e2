"""The two kernels at the ends of td_vae_decode, alone and bit for bit (td_vae_latents_to_nhwc_bf16, td_vae_image_finalize: csrc/vae_kernels.hip
td_latents_to_nhwc_kernel / td_image_finalize_kernel behind entries of their own; the engine launches the same kernels).  Both are written as
exact restatements of bf16 torch statements, so the reference is that statement run by torch on the CPU and the comparison is on bits:

  latents_to_nhwc   (unpack_latents(packed, h, w) / scaling_factor) + shift_factor     on bf16 tensors ([ext] diffusers pipeline_flux.py), in
                    NHWC with channels >= C zero.  The quotient rounds to bf16, then the sum with bf16(shift_factor) rounds.
  image_finalize    ((x / 2 + 0.5).clamp(0, 1).float() * 255).round().to(uint8)       oracle/vae_ref.latents_to_image's statement, and the
                    input's own bits in [3, P] order.

An exact bf16 rounding tie of the fp32 quotient x / scaling_factor exists for no finite bf16 x with either divisor used here (0.3611, 0.13025:
their fp32 values have full-width significands; asserted below), so the inputs carry the x whose fp32 quotients lie NEAREST a tie, the x whose
second step -- bf16(quotient) + bf16(shift) in fp32 -- lies exactly on one, +-0 and the largest finite bf16 (whose quotient overflows to inf in
both), and one further case feeds every finite bf16 bit pattern through the kernel.
"""
import pytest
import torch

from oracle import flux_ref as R

pytestmark = pytest.mark.gpu

FACTORS = [(0.3611, 0.1159), (0.13025, 0.0)]      # (scaling_factor, shift_factor): FLUX.1's VAE, SDXL's


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _finite_bf16():
    """Every finite bf16 bit pattern, in bit order: 65280 values."""
    allb = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    x = allb[torch.isfinite(allb)]
    assert x.numel() == 65280
    return x


def _plants(sf, shift):
    """+-0, +-largest finite, the 8 finite bf16 x whose fp32 quotient x / sf lies nearest a bf16 rounding tie, and up to 8 whose second step's
    fp32 sum lies exactly on one."""
    x = _finite_bf16()
    q = x.float() / torch.tensor(sf, dtype=torch.float32)
    ok = torch.isfinite(q) & (q.abs() >= 2.0 ** -120)
    dist = ((q.view(torch.int32) & 0xFFFF) - 0x8000).abs()
    assert int(dist[ok].min()) > 0, "an exact tie of the quotient exists after all: plant it"
    near = x[ok][torch.argsort(dist[ok])[:8]]
    s = q.bfloat16().float() + torch.tensor(shift).bfloat16().float()
    tie2 = x[ok & ((s.view(torch.int32) & 0xFFFF) == 0x8000)][:8]
    edge = torch.tensor([0.0, -0.0, 3.3895e38, -3.3895e38]).bfloat16()
    return torch.cat([edge, near, tie2])


def _latents_ref(packed, h, w, sf, shift):
    z = (R.unpack_latents(packed[None], h, w) / sf) + shift          # the statement, on bf16 tensors
    assert z.dtype == torch.bfloat16
    return z[0].permute(1, 2, 0).reshape(h * w, -1).contiguous()


def _check_latents(hip, packed, h, w, Cpad, sf, shift):
    C = packed.shape[1] // 4
    got = hip.vae_latents_to_nhwc(packed.cuda(), h, w, Cpad, sf, shift)
    torch.cuda.synchronize()
    assert got.shape == (h * w, Cpad)
    want = _latents_ref(packed, h, w, sf, shift)
    bad = _bits(got[:, :C]) != _bits(want)
    assert not bool(bad.any()), (int(bad.sum()), got[:, :C].cpu()[bad][:4], want[bad][:4])
    assert not bool(_bits(got[:, C:]).any()), "channels >= C are not +0.0"


@pytest.mark.parametrize("sf,shift", FACTORS)
@pytest.mark.parametrize("Cpad", [16, 64])
@pytest.mark.parametrize("h,w", [(2, 2), (6, 10), (16, 24)])
def test_latents_to_nhwc_bit_exact(hip, h, w, Cpad, sf, shift):
    C = 16
    g = torch.Generator().manual_seed(h * 100 + w)
    packed = (torch.randn((h // 2) * (w // 2), 4 * C, generator=g) * 2).bfloat16()
    p = _plants(sf, shift)
    assert p.numel() <= packed.numel()
    packed.view(-1)[torch.randperm(packed.numel(), generator=g)[:p.numel()]] = p      # scattered over tokens, channels and 2x2 positions
    _check_latents(hip, packed, h, w, Cpad, sf, shift)


@pytest.mark.parametrize("sf,shift", FACTORS)
def test_latents_to_nhwc_every_finite_bf16(hip, sf, shift):
    """64 x 64 latents of 16 channels hold 65536 values: every finite bf16 bit pattern once, and 256 zeros."""
    h = w = 64
    packed = torch.zeros((h // 2) * (w // 2) * 64, dtype=torch.bfloat16)
    packed[:65280] = _finite_bf16()
    _check_latents(hip, packed.view(-1, 64), h, w, 16, sf, shift)


def _u8_ref(x):
    return ((x / 2 + 0.5).clamp(0, 1).float() * 255).round().to(torch.uint8)      # on a bf16 x


SENTINEL = 0x7FC1      # a NaN no input holds: pad channels carry it, and it must reach neither output


def _padded(live, Cpad):
    x = torch.full((live.shape[0], Cpad), SENTINEL, dtype=torch.int16).view(torch.bfloat16)
    x[:, :3] = live
    return x


def test_image_finalize_every_finite_bf16(hip):
    live = _finite_bf16().view(-1, 3)                                   # P = 21760 pixels, every finite bf16 bit pattern once
    P = live.shape[0]
    # what the statement does, checked here: v * 255 is exact in fp32 for every bf16 v in [0, 1], all 256 codes occur, and the one half-way
    # product, 127.5, goes to 128 under round-half-even (torch, rintf) and under round-half-up alike
    den = (live / 2 + 0.5).clamp(0, 1)
    prod = den.float() * 255
    assert torch.equal(prod.double(), den.double() * 255)
    half = prod[(prod - prod.floor()) == 0.5]
    assert half.numel() > 0 and bool((half == 127.5).all())
    assert float(torch.round(torch.tensor(127.5))) == 128.0 == float(torch.floor(torch.tensor(127.5) + 0.5))
    want8 = _u8_ref(live)
    assert want8.unique().numel() == 256
    x = _padded(live, 8).cuda()
    u8, chw = hip.vae_image_finalize(x)
    u8_only, none_c = hip.vae_image_finalize(x, chw=False)
    none_8, chw_only = hip.vae_image_finalize(x, u8=False)
    torch.cuda.synchronize()
    assert none_c is None and none_8 is None
    assert u8.shape == (P, 3) and chw.shape == (3, P)
    bad = u8.cpu() != want8
    assert not bool(bad.any()), (int(bad.sum()), live[bad][:4], u8.cpu()[bad][:4], want8[bad][:4])
    assert torch.equal(_bits(chw), _bits(live.t()))
    assert torch.equal(u8_only.cpu(), want8) and torch.equal(_bits(chw_only), _bits(live.t()))


def test_image_finalize_row_stride_64(hip):
    """The engine's own layout where the last conv writes 64-channel rows: three live channels per 64."""
    g = torch.Generator().manual_seed(9)
    live = (torch.randn(1000, 3, generator=g) * 0.8).bfloat16()
    u8, chw = hip.vae_image_finalize(_padded(live, 64).cuda())
    torch.cuda.synchronize()
    assert torch.equal(u8.cpu(), _u8_ref(live)) and torch.equal(_bits(chw), _bits(live.t()))


def test_image_finalize_nan_and_inf(hip):
    """+-inf have a defined image (255 / 0).  A NaN's uint8 cast is undefined in the reference: the kernel must write SOME byte there -- shown by
    two runs over outputs prefilled with different bytes agreeing -- and carry the NaN's bits to the bf16 output."""
    pats = torch.tensor([0x7FC0, 0xFFC0 - 65536, 0x7F81, 0x7FFF, 0x7F80, 0xFF80 - 65536], dtype=torch.int16).view(torch.bfloat16)
    live = torch.zeros(4, 3, dtype=torch.bfloat16)
    live.view(-1)[:6] = pats
    x = _padded(live, 8).cuda()
    outs = []
    for fill in (0x00, 0xFF):
        u8 = torch.full((4, 3), fill, dtype=torch.uint8, device="cuda")
        chw = torch.full((3, 4), fill, dtype=torch.uint8, device="cuda").repeat_interleave(2, dim=1).view(torch.bfloat16)
        hip.check(hip.lib().td_vae_image_finalize(hip.ptr(x), 4, 8, hip.ptr(u8), hip.ptr(chw), hip.stream_ptr()))
        torch.cuda.synchronize()
        outs.append(u8.cpu())
        assert torch.equal(_bits(chw), _bits(live.t()))
    assert torch.equal(outs[0], outs[1])
    assert outs[0].view(-1)[4:].tolist() == [255, 0, 128, 128, 128, 128, 128, 128]      # +inf, -inf, then the zeros: 0 / 2 + 0.5 -> 127.5 -> 128
