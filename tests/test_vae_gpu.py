"""GPU parity of the VAE decoder kernels / engine (td_conv3x3_nhwc_bf16, td_groupnorm_nhwc_bf16, td_vae_decode)
against the CPU oracle (oracle/vae_ref.py: F.conv2d / F.group_norm / SDPA in bf16 = the reference's arithmetic).

Tolerances: conv / groupnorm single ops <= 2^-6 of the output scale (bf16 output, fp32 accumulate, different
summation order); the tiny 2-block decoder end to end: relative RMSE <= 3e-2 vs the bf16 oracle and uint8 pixels
within 1e-2 RMSE on the [0,1] scale (the north-star pixel bar).

td_groupnorm_nhwc_bf16 against float64 (test_groupnorm_vs_float64): reference = float64 GroupNorm of the bf16 input, t = bf16((x - mean)
rstd gamma + beta), then y = bf16(silu(t)) in float64 when silu is set -- the kernel's two rounding points.  Per-element tolerance:
  tol_t = ulp(|t| + S) + S,      tol_y = ulp(|y| + d) + d,  d = |silu'(t)| tol_t      (ulp(r) = one bf16 ulp of r)
One ulp at each of the two rounding points, taken at the largest magnitude the rounded value can have (the reference's plus what
reaches it from upstream): next to a power of two the kernel's value may lie in the binade above the reference's, where the ulp is
twice as large -- e.g. t one ulp lower takes silu(t) from -0.031188 to -0.031417, which round to -0.0311279 and -0.0314941, three
ulps of the reference apart but one ulp of the upper binade plus silu' ulp(t).
  S = (L + 8) 2^-24 rstd |gamma| (mean|x| + 1.5 |x - mean| E[x^2] / var)
S is what the fp32 statistics may cost, derived as tests/test_norms_gpu.py derives its term.  td_gn_partial_kernel adds every value
into fp32 chains of length at most L = ceil(ppb / ppp) + 8 + ppp nj (the thread's pixels, its 8-channel sum, then ppp nj sub-sums in
the block's fixed-order sum; ppb pixels per block, ppp = 256 / (C/8) pixels per pass, nj = max(cpg / 8, 1)); the block partials are
added in double.  Worst-case rounding of such a sum is L 2^-24 of the sum of magnitudes: the mean is off by <= L 2^-24 mean|x|, which
moves t by that times rstd |gamma|.  The variance is ONE-PASS, var = E[x^2] - mean^2: E[x^2] is off by L 2^-24 E[x^2] and mean^2 by
2 |mean| L 2^-24 mean|x| <= 2 L 2^-24 E[x^2], so var is off by 3 L 2^-24 E[x^2] -- RELATIVE to var that is the cancellation factor
E[x^2] / var -- and rstd by half of it, which moves t by 1.5 L 2^-24 (E[x^2] / var) |x - mean| rstd |gamma|.  The factor stays in the
formula so that it is visible what the one-pass form is being allowed: ~1 for centred data, 1e4 at mean / std = 100.  The + 8 covers
the fp32 casts of mean and rstd and the fp32 output expression.  Measured on MI355X, max error x the bound: 0 (the four shapes of <= 128 pixels with <= 64 channels: every bit right) to 0.999 without SiLU -- an element
whose rounding flipped -- and to 0.81 with it.

DC-offset inputs (test_groupnorm_dc_offset_groups) take their bar from the reference's own arithmetic instead: see the test.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import flux_ref as R
from oracle import vae_ref as V

pytestmark = pytest.mark.gpu


def _close(got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max() / ref.abs().max()
    assert err < tol, f"rel-to-scale err {err:.3e}"


@pytest.mark.parametrize("H,W,Cin,Cout,up,res", [(16, 16, 64, 64, False, False), (24, 40, 128, 256, False, True),
                                                 (32, 32, 64, 128, True, False), (18, 22, 64, 8, False, False)])
def test_conv3x3_implicit_gemm(hip, H, W, Cin, Cout, up, res):
    """One number against the output scale; the per-element bounds and the edge shapes are in tests/test_vae_conv_fp64_gpu.py."""
    g = torch.Generator().manual_seed(H * W + Cin)
    Hin, Win = (H // 2, W // 2) if up else (H, W)
    x = torch.randn(1, Cin, Hin, Win, generator=g).bfloat16()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).bfloat16()
    b = torch.randn(Cout, generator=g).bfloat16()
    r = torch.randn(1, Cout, H, W, generator=g).bfloat16() if res else None
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest").bfloat16() if up else x
    ref = F.conv2d(xin.float(), w.float(), b.float(), padding=1).bfloat16()
    if res:
        ref = (ref.float() + r.float()).bfloat16()
    nhwc = lambda t: t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()
    wp = hip.conv3x3_pack_weight(w.cuda())
    y = hip.conv3x3_nhwc(nhwc(x).cuda(), wp, b.cuda(), H, W, Cout, res=nhwc(r).cuda() if res else None, upsample2x=up)
    torch.cuda.synchronize()
    _close(y, nhwc(ref), 2.0 ** -6)


@pytest.mark.parametrize("P,C,silu", [(256, 64, True), (4096, 128, False), (1000, 512, True)])
def test_groupnorm_silu_nhwc(hip, P, C, silu):
    g = torch.Generator().manual_seed(P + C)
    x = (torch.randn(P, C, generator=g) * 2 + 0.3).bfloat16()
    ga, be = (1 + 0.1 * torch.randn(C, generator=g)).bfloat16(), (0.1 * torch.randn(C, generator=g)).bfloat16()
    ref = F.group_norm(x.t()[None], 32, ga, be, eps=1e-6)
    if silu:
        ref = F.silu(ref)
    y = hip.groupnorm_nhwc(x.cuda(), ga.cuda(), be.cuda(), 32, 1e-6, silu)
    torch.cuda.synchronize()
    _close(y, ref[0].t(), 2.0 ** -6)


def _ulp(r):
    a = r.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _gn_chain(P, C, G):
    """Longest fp32 addition chain of td_gn_partial_kernel for this shape (the launcher's block split restated)."""
    nblocks = min(1024, (P + 63) // 64)
    ppb = -(-P // nblocks)
    ppp = 256 // (C // 8)
    nj = max(C // G // 8, 1)
    return -(-ppb // ppp) + 8 + ppp * nj


def _gn_stats64(x, G):
    """float64 per-element mean, biased variance and E[x^2] of x [P, C] over (all pixels, the channels of the group)."""
    P, C = x.shape
    xg = x.double().reshape(P, G, C // G)
    mean = xg.mean(dim=(0, 2), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(0, 2), keepdim=True)
    ex2 = (xg * xg).mean(dim=(0, 2), keepdim=True)
    absx = xg.abs().mean(dim=(0, 2), keepdim=True)
    full = lambda t: t.expand(P, G, C // G).reshape(P, C)
    return full(mean), full(var), full(ex2), full(absx)


def _gn_ref(x, ga, be, G, eps, silu):
    """float64 reference and its per-element tolerance (derivation: module docstring)."""
    P, C = x.shape
    mean, var, ex2, absx = _gn_stats64(x, G)
    rstd = 1.0 / torch.sqrt(var + eps)
    xd, gd = x.double(), ga.double()[None, :]
    t = ((xd - mean) * rstd * gd + be.double()[None, :]).bfloat16().double()
    S = (_gn_chain(P, C, G) + 8) * 2.0 ** -24 * rstd * gd.abs() * (absx + 1.5 * (xd - mean).abs() * ex2 / (var + eps))
    tol = _ulp(t.abs() + S) + S
    if not silu:
        return t, tol
    sg = torch.sigmoid(t)
    y = (t * sg).bfloat16().double()
    d = (sg * (1.0 + t * (1.0 - sg))).abs() * tol
    return y, _ulp(y.abs() + d) + d


def _gn_check(got, ref, tol, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    bad = err > tol
    print(f"{what}: max error {float((err / tol).max()):.3f} x the bound")
    if bad.any():
        i = int(torch.argmax(err / tol))
        r, c = divmod(i, ref.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements beyond the bound; worst pixel {r} channel {c}: got "
                             f"{float(got[r, c]):.6g} ref {float(ref[r, c]):.6g} ({float(err[r, c] / tol[r, c]):.3g} x the bound)")


def _gn_affine(C, g):
    """gamma and beta with a visible spread (a channel-index error shows)."""
    return (1.0 + 0.5 * torch.randn(C, generator=g)).bfloat16(), (0.7 * torch.randn(C, generator=g)).bfloat16()


# (P, C, G): a single pixel; cpg = 1 / 2 (two blocks) / 4: the sub-group path of a thread's 8 channels; cpg = 8, 16, 64: the nj path, the last
# with tpp = 256 threads per pixel and one pixel per pass; cpg = 24 with tpp = 24 not dividing 256 (16 idle threads); G = 64 and G = 1;
# 70000 pixels: the 1024-block cap, 69 pixels per block, the last 9 blocks empty
GN_SHAPES = [(1, 64, 32), (63, 32, 32), (65, 64, 32), (1000, 128, 32), (257, 256, 32), (300, 512, 32), (64, 2048, 32), (100, 192, 8),
             (128, 64, 64), (500, 64, 1), (70000, 64, 32)]


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("P,C,G", GN_SHAPES)
def test_groupnorm_vs_float64(hip, P, C, G, silu):
    """Every index path of the statistics kernel against float64, every group with its own mean (+-3) and spread (0.5 .. 2.5)."""
    g = torch.Generator().manual_seed(P * 31 + C + G)
    gm = (torch.rand(G, generator=g) * 6.0 - 3.0).repeat_interleave(C // G)
    gs = (0.5 + 2.0 * torch.rand(G, generator=g)).repeat_interleave(C // G)
    x = (torch.randn(P, C, generator=g) * gs[None, :] + gm[None, :]).bfloat16()
    ga, be = _gn_affine(C, g)
    ref, tol = _gn_ref(x, ga, be, G, 1e-6, silu)
    y = hip.groupnorm_nhwc(x.cuda(), ga.cuda(), be.cuda(), G, 1e-6, silu)
    torch.cuda.synchronize()
    _gn_check(y, ref, tol, f"groupnorm P={P} C={C} G={G} silu={silu}")


# (mean, std) of the groups, in turn: mean / std from 32 to 100 (beyond ~256 the spread is no longer representable in bf16)
GN_DC = [(16.0, 0.5), (50.0, 1.0), (100.0, 2.0), (200.0, 2.0), (-200.0, 4.0)]


@pytest.mark.parametrize("P,C", [(4096, 128), (16384, 512)])
def test_groupnorm_dc_offset_groups(hip, P, C):
    """Groups whose mean is large next to their spread, where the one-pass variance E[x^2] - mean^2 over fp32 partial sums is at risk
    (the generic LayerNorm kernel is guarded against the same in tests/test_norms_gpu.py).  The bar is the reference's own arithmetic:
    F.group_norm of the same input in fp32 on the CPU, rounded to bf16.  Both implementations are measured against float64 GroupNorm
    rounded to bf16, in bf16 ulps of that reference over the elements with |ref| > 0.1; the kernel's worst error may exceed the fp32
    implementation's by at most ONE ulp (two valid fp32 statistics can flip one rounding).
    Measured on MI355X: (4096, 128): kernel 1.00 ulp, fp32 F.group_norm 1.00 ulp; (16384, 512): kernel 1.00 ulp, fp32 F.group_norm 1.00 ulp
    -- the one-pass form loses nothing at these offsets, so td_gn_partial_kernel stays as it is."""
    G = 32
    g = torch.Generator().manual_seed(P + C)
    gm = torch.tensor([GN_DC[i % len(GN_DC)][0] for i in range(G)]).repeat_interleave(C // G)
    gs = torch.tensor([GN_DC[i % len(GN_DC)][1] for i in range(G)]).repeat_interleave(C // G)
    x = (torch.randn(P, C, generator=g) * gs[None, :] + gm[None, :]).bfloat16()
    ga, be = _gn_affine(C, g)
    mean, var, _, _ = _gn_stats64(x, G)
    ref = ((x.double() - mean) / torch.sqrt(var + 1e-6) * ga.double()[None, :] + be.double()[None, :]).bfloat16().double()
    cpu = F.group_norm(x.float().t()[None], G, ga.float(), be.float(), eps=1e-6)[0].t().bfloat16().double()
    y = hip.groupnorm_nhwc(x.cuda(), ga.cuda(), be.cuda(), G, 1e-6, False)
    torch.cuda.synchronize()
    got = y.double().cpu()
    assert torch.isfinite(got).all()
    sel = ref.abs() > 0.1
    u = _ulp(ref)
    e_kernel = float(((got - ref).abs() / u)[sel].max())
    e_cpu = float(((cpu - ref).abs() / u)[sel].max())
    print(f"groupnorm DC-offset groups P={P} C={C}: worst error {e_kernel:.2f} bf16 ulp (kernel), {e_cpu:.2f} bf16 ulp (fp32 F.group_norm on the CPU)")
    assert e_kernel <= e_cpu + 1.0, f"kernel {e_kernel:.2f} ulp vs fp32 reference arithmetic {e_cpu:.2f} ulp"


def _tiny_vae(seed):
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder
    cfg = V.tiny_config()
    sd = V.init_weights(cfg, seed=seed)
    m = AutoencoderKLDecoder(AutoencoderKLConfig(block_out_channels=cfg.block_out_channels), max_latent_size=(16, 16))
    m.load_state_dict(sd)
    return cfg, sd, m


@pytest.mark.parametrize("h,w", [(8, 8), (16, 12)])
def test_vae_decode_matches_oracle(hip, h, w):
    cfg, sd, m = _tiny_vae(seed=h)
    g = torch.Generator().manual_seed(w)
    packed = (torch.randn(1, (h // 2) * (w // 2), 64, generator=g) * 0.8).bfloat16()
    ref_img, ref_u8 = V.latents_to_image(sd, cfg, packed, h, w)
    img = m.decode_packed(packed[0].cuda(), h, w, output_type="pt")
    u8 = m.decode_packed(packed[0].cuda(), h, w, output_type="np")
    torch.cuda.synchronize()
    assert img.shape == (3, 2 * h, 2 * w) and u8.shape == (2 * h, 2 * w, 3) and u8.dtype == torch.uint8
    rel = float((img.float().cpu() - ref_img[0].float()).pow(2).mean().sqrt() / ref_img.float().pow(2).mean().sqrt())
    px = float(((u8.float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"vae tiny {h}x{w}: rel-RMSE {rel:.4f}, pixel RMSE {px:.5f}")
    assert rel < 3e-2 and px < 1e-2


def test_pipeline_returns_pil_image(hip):
    """FluxPipelineRewritePrompt(...).images[0] is a PIL image once a VAE is attached (the drivers .save() it)."""
    from thinkdiff.models.flux_prompt import FluxPipelineRewritePrompt
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel, FluxTransformerConfig
    cfgv, sdv, vae = _tiny_vae(seed=3)
    fc = R.tiny_config(num_layers=1, num_single_layers=1)
    tr = FluxTransformer2DModel(FluxTransformerConfig(num_layers=1, num_single_layers=1, num_attention_heads=fc.num_attention_heads,
                                                      joint_attention_dim=fc.joint_attention_dim, pooled_projection_dim=fc.pooled_projection_dim),
                                max_img_tokens=64, max_txt_tokens=32, max_steps=4)
    tr.load_state_dict(R.init_weights(fc, seed=1))
    pipe = FluxPipelineRewritePrompt(transformer=tr, vae=vae)
    pipe.vae_scale_factor = 4   # 2-block tiny VAE: image = 2 x latent, latent = 2 x packed grid
    g = torch.Generator().manual_seed(0)
    out = pipe(prompt_embeds=torch.randn(1, 16, fc.joint_attention_dim, generator=g).bfloat16().cuda(),
               pooled_prompt_embeds=torch.randn(1, fc.pooled_projection_dim, generator=g).bfloat16().cuda(),
               height=32, width=32, num_inference_steps=2, guidance_scale=3.5)
    assert out.images[0].size == (32, 32) and out.images[0].mode == "RGB"


def test_vae_full_architecture_small_image(hip):
    """The FLUX.1 VAE decoder architecture at full width (block_out_channels 128/256/512/512, 2 layers per block, the
    512-channel single-head mid-block attention) on a 16x16 latent -> 128x128 image, against the oracle."""
    from thinkdiff.models.flux_vae import AutoencoderKLConfig, AutoencoderKLDecoder
    cfg = V.VaeConfig()
    sd = V.init_weights(cfg, seed=3)
    m = AutoencoderKLDecoder(AutoencoderKLConfig(), max_latent_size=(16, 16))
    m.load_state_dict(sd)
    h = w = 16
    g = torch.Generator().manual_seed(11)
    packed = (torch.randn(1, (h // 2) * (w // 2), 64, generator=g) * 0.8).bfloat16()
    ref_img, ref_u8 = V.latents_to_image(sd, cfg, packed, h, w)
    img = m.decode_packed(packed[0].cuda(), h, w, output_type="pt")
    u8 = m.decode_packed(packed[0].cuda(), h, w, output_type="np")
    torch.cuda.synchronize()
    assert img.shape == (3, 8 * h, 8 * w) and u8.shape == (8 * h, 8 * w, 3)
    rel = float((img.float().cpu() - ref_img[0].float()).pow(2).mean().sqrt() / ref_img.float().pow(2).mean().sqrt())
    px = float(((u8.float().cpu() - ref_u8[0].float()) / 255).pow(2).mean().sqrt())
    print(f"vae full architecture 16x16 latent: rel-RMSE {rel:.4f}, pixel RMSE {px:.5f}")
    assert rel < 3e-2 and px < 1e-2
