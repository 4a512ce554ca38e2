"""Generic row normalisation (td_layernorm_bf16: the norm of CLIP, EVA-ViT and the Qwen2-VL ViT) against float64 nn.LayerNorm /
T5LayerNorm, and the FLUX norm kernel (td_norm_rows_bf16) on rows with a large common offset.

Reference: the bf16 input in float64; LayerNorm = (x - mean) / sqrt(var + eps) * w + b rounded once to bf16 (nn.LayerNorm on bf16
is one fp32 expression); T5LayerNorm = bf16(bf16(x / sqrt(mean(x^2) + eps)) * w) (cast to the weight dtype, then the weight).

Tolerance, per element: one bf16 ulp of the reference at every rounding point (for T5LayerNorm with a weight, that adds |w| times
one ulp of the inner bf16 value), plus what the fp32 row mean can be off by, moved through the output: (D/64 + 8) 2^-24 mean|x|
rstd |w| -- the worst-case rounding of a sum whose longest chain is D/64 lane additions, 6 butterfly steps and the division.  It
matters only next to y = 0 (x within a few fp32 ulps of the mean); on the DC-offset rows it is still >100x smaller than the
error of a one-pass variance E[x^2] - mean^2, which moves every element of the row by several bf16 ulps.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


from flux_rowops_common import _check, _ref, _ulp  # noqa: F401  (the float64 reference, ulp and check, shared with the FLUX row-kernel tests)


@pytest.mark.parametrize("D", [8, 520, 768, 1024, 1280, 1408, 4096])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 257])
def test_layernorm_generic_vs_float64(hip, D, rows):
    """Every mode on one shape: LayerNorm with w and b, w only, b only, neither; T5LayerNorm with and without w; eps 1e-5 and 1e-6.
    x and y are strided (ld > D) and y's pad columns must stay untouched.  D = 520 leaves the last 512-column sweep partial; a
    block holds 4 rows, so 1, 3, 4, 5 and 257 rows cover partial and full blocks."""
    g = torch.Generator().manual_seed(D * 17 + rows)
    ldx, ldy = D + 24, D + 16
    xs = (torch.randn(rows, ldx, generator=g) * 1.5 + 0.3).bfloat16()
    w = (1.0 + 0.3 * torch.randn(D, generator=g)).bfloat16()
    b = (0.5 * torch.randn(D, generator=g)).bfloat16()
    xd = xs.cuda()[:, :D]
    for rms, use_w, use_b, eps in [(False, True, True, 1e-5), (False, True, False, 1e-6), (False, False, True, 1e-5),
                                   (False, False, False, 1e-6), (True, True, False, 1e-6), (True, False, False, 1e-5)]:
        ww, bb = (w if use_w else None), (b if use_b else None)
        yfull = torch.full((rows, ldy), -3.0, dtype=torch.bfloat16, device="cuda")
        hip.layernorm(xd, None if ww is None else ww.cuda(), None if bb is None else bb.cuda(), eps=eps, rms=rms, out=yfull[:, :D])
        torch.cuda.synchronize()
        ref, tol = _ref(xs[:, :D], ww, bb, eps, rms)
        what = f"layernorm D={D} rows={rows} rms={rms} w={use_w} b={use_b} eps={eps}"
        _check(yfull[:, :D], ref, tol, what)
        assert (yfull[:, D:].cpu().float() == -3.0).all(), what + ": pad columns of y written"


# (mean, std) of the DC-offset rows: mean / std from 1 to 3000
DC_ROWS = [(1.0, 1.0), (10.0, 1.0), (64.0, 0.25), (256.0, 1.0), (300.0, 0.5), (600.0, 1.0), (1000.0, 2.0), (3000.0, 4.0), (-3000.0, 16.0)]


def _dc_rows(D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([m + s * torch.randn(D, generator=g) for m, s in DC_ROWS]).bfloat16()
    assert (x.float().std(dim=1) > 0).all()
    return x


@pytest.mark.parametrize("D", [768, 1280, 1408])
def test_layernorm_generic_dc_offset_rows(hip, D):
    """Rows whose mean is large next to their spread: the variance must come from x - mean, not from E[x^2] - mean^2 (which loses
    the spread to fp32 cancellation: rstd wrong by far more than one bf16 ulp)."""
    x = _dc_rows(D, D)
    g = torch.Generator().manual_seed(D + 1)
    w = (1.0 + 0.3 * torch.randn(D, generator=g)).bfloat16()
    b = (0.5 * torch.randn(D, generator=g)).bfloat16()
    for ww, bb in [(None, None), (w, b)]:
        y = hip.layernorm(x.cuda(), None if ww is None else ww.cuda(), None if bb is None else bb.cuda(), eps=1e-5)
        torch.cuda.synchronize()
        ref, tol = _ref(x, ww, bb, 1e-5, False)
        _check(y, ref, tol, f"layernorm DC-offset rows D={D} affine={ww is not None}")


@pytest.mark.parametrize("D", [1024, 1536])
def test_flux_norm_rows_dc_offset_rows(hip, D):
    """The same rows through the FLUX norm kernel (td_norm_rows_bf16: D a multiple of 512, LayerNorm without affine, eps 1e-6),
    which subtracts the mean before squaring."""
    x = _dc_rows(D, D)
    y = hip.norm_rows(x.cuda(), eps=1e-6)
    torch.cuda.synchronize()
    ref, tol = _ref(x, None, None, 1e-6, False)
    _check(y, ref, tol, f"norm_rows DC-offset rows D={D}")
