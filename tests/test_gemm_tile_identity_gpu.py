"""The 256x256 (tile_cfg 0) and the 288x192 (tile_cfg 3) GEMM tiles give the same bits: both contract K in the same k-tile and k-step order on the
same MFMA and round at the same points of the epilogue.  That is what lets the engine choose between them by CU time when images share the chip
(td_gemm_plan; TD_GEMM_SHARED_TILES=0 restores the lone-launch choice) without changing an image: checked on the launch forms the FLUX blocks use,
and on two contexts in flight through td_flux_denoise_multi, whose traced launches must move from the 288x192 category to the 256x256 one."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCH = "TD_GEMM_SHARED_TILES"


def _problem(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).bfloat16().cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16().cuda()
    b = torch.randn(N, generator=g).bfloat16().cuda()
    gate = torch.randn(N, generator=g).bfloat16().cuda()
    y = torch.randn(M, N, generator=g).bfloat16().cuda()      # what an in-place residual launch finds in its output
    return x, w, b, gate, y


def _run(hip, form, cfg, p0, p1=None):
    x0, w0, b0, g0, y0 = p0
    y0 = y0.clone()
    x1 = w1 = b1 = g1 = y1 = None
    if p1 is not None:
        x1, w1, b1, g1, y1 = p1
        y1 = y1.clone()
    if form == "bias":
        hip.linear_grouped2(x0, w0, b0, y0, x1, w1, b1, y1, tile_cfg=cfg)
    elif form == "gelu":
        hip.linear_grouped2(x0, w0, b0, y0, x1, w1, b1, y1, act=hip.ACT_GELU_TANH, tile_cfg=cfg)
    else:      # y += gate * (x W^T + b), in place
        hip.linear_grouped2(x0, w0, b0, y0, x1, w1, b1, y1, gate0=g0, res0=y0, gate1=g1, res1=y1, tile_cfg=cfg)
    torch.cuda.synchronize()
    return y0, y1


# M = 300: a ragged second row tile of both shapes (44 / 12 rows); N = 392, 200: ragged last column tiles; 260 + 70 rows: the grouped launch of the
# double blocks, each problem with a ragged last row tile
@pytest.mark.parametrize("form", ["bias", "gelu", "gated_residual"])
@pytest.mark.parametrize("M,M1,N,K", [(300, 0, 392, 192), (577, 0, 200, 128), (260, 70, 392, 192), (260, 70, 200, 128)])
def test_tiles_agree_bit_for_bit(hip, form, M, M1, N, K):
    p0 = _problem(M, N, K, 11)
    p1 = _problem(M1, N, K, 12) if M1 else None
    a0, a1 = _run(hip, form, 0, p0, p1)
    c0, c1 = _run(hip, form, 3, p0, p1)
    assert torch.isfinite(a0.float()).all() and not torch.equal(a0, p0[4])
    assert torch.equal(a0, c0)
    if M1:
        assert not torch.equal(a1, p1[4]) and torch.equal(a1, c1)


def test_tiles_agree_at_the_single_blocks_proj_out(hip):
    """4289 x 3072 x 15360, gated residual in place: the launch the shared-chip choice moves."""
    p0 = _problem(4289, 3072, 15360, 13)
    a0, _ = _run(hip, "gated_residual", 0, p0)
    c0, _ = _run(hip, "gated_residual", 3, p0)
    auto, _ = _run(hip, "gated_residual", -1, p0)
    assert torch.isfinite(a0.float()).all() and not torch.equal(a0, p0[4])
    assert torch.equal(a0, c0) and torch.equal(a0, auto)


@pytest.fixture
def switch():
    prev = os.environ.pop(SWITCH, None)
    yield
    os.environ.pop(SWITCH, None)
    if prev is not None:
        os.environ[SWITCH] = prev


def test_two_images_in_flight_same_latents_other_tile(hip, switch):
    """1 double + 1 single block at D = 3072, 4096 image + 193 text tokens, two contexts, 2 steps: per context and step, ff.net.2 (K = 12288, image +
    text rows in one launch) and the single block's proj_out (K = 15360) are the lone-launch rule's 288x192 launches."""
    from thinkdiff.models.flux_transformer import FluxTransformer2DModel
    S, T, steps = 4096, 193, 2
    m = FluxTransformer2DModel(num_layers=1, num_single_layers=1, max_img_tokens=S, max_txt_tokens=256, max_steps=4).init_random(seed=5)
    ctxs = [m, m.fork()]
    g = torch.Generator().manual_seed(6)
    ids = torch.zeros(64, 64, 3)
    ids[..., 1] += torch.arange(64)[:, None]
    ids[..., 2] += torch.arange(64)[None, :]
    sig = [1.0, 0.6, 0.0]
    for c in ctxs:
        c.set_condition((0.1 * torch.randn(T, 4096, generator=g)).bfloat16().cuda(), torch.randn(768, generator=g).bfloat16().cuda(), ids.reshape(-1, 3))
        c.set_timesteps([s * 1000.0 for s in sig[:-1]], 3500.0)
    lat = [torch.randn(S, 64, generator=g).bfloat16().cuda() for _ in ctxs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()

    def run(value):
        os.environ[SWITCH] = value
        xs = [x.clone() for x in lat]
        ctxs[0].trace_begin(512)
        FluxTransformer2DModel.denoise_multi(ctxs, xs, sig, streams)
        torch.cuda.synchronize()
        tr = ctxs[0].trace_end()
        return xs, {k: v["launches"] for k, v in tr.items()}

    x_old, n_old = run("0")
    x_new, n_new = run("1")
    print("launches per category, lone-launch rule:", n_old, "| CU-time choice:", n_new)
    for a, b, x in zip(x_old, x_new, lat):
        assert torch.isfinite(a.float()).all() and not torch.equal(a, x)
        assert torch.equal(a, b)
    assert not torch.equal(x_old[0], x_old[1])
    moved = 2 * steps      # ff.net.2 + proj_out, per step
    assert n_old["gemm_288x192"] == moved and n_new["gemm_288x192"] == 0
    assert n_new["gemm_256x256"] == n_old["gemm_256x256"] + moved
    assert sum(n_new.values()) == sum(n_old.values())
    assert all(n_new[k] == n_old[k] for k in n_old if k not in ("gemm_288x192", "gemm_256x256"))
