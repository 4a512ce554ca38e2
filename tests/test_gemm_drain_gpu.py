"""The persistent walk of the 256x256 bf16 GEMM tile (td_gemm_bf16_drain_kernel: a workgroup walks several tiles and stores part of each
tile's output from inside the next tile's main loop) against the one-tile-per-workgroup launch of the same problem (TD_GEMM_DRAIN=0, read
per launch), bit for bit.  Every output buffer is compared whole, rows and pad columns the launch must not touch included.  The
one-tile-per-workgroup launch itself is held against fp32 references by tests/test_gemm_gpu.py.

td_linear_drain_bf16 forces the 256x256 tile and bounds the walking workgroups, so that these small problems walk several tiles each.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 8          # columns behind N in every output row: never written


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).bfloat16().cuda()


def _both(launch):
    """launch() -> list of output tensors; run it with the walk off, then on."""
    prev = os.environ.get("TD_GEMM_DRAIN")
    try:
        os.environ["TD_GEMM_DRAIN"] = "0"
        ref = launch()
        os.environ.pop("TD_GEMM_DRAIN")
        got = launch()
        torch.cuda.synchronize()
    finally:
        if prev is None:
            os.environ.pop("TD_GEMM_DRAIN", None)
        else:
            os.environ["TD_GEMM_DRAIN"] = prev
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(b.float()).all()
        assert torch.equal(a, b), f"output {i}: {(a != b).sum().item()} of {a.numel()} elements differ"


def _out(M, N, fill=0.5):
    buf = torch.full((M + 3, N + PAD), fill, dtype=torch.bfloat16, device="cuda")      # three guard rows behind M
    return buf, buf[:M, :N]


@pytest.mark.parametrize("K", [128, 64])
def test_one_workgroup_walks_six_tiles_short_k(hip, K):
    """M = 513: the last row tile holds one row (the ragged loop).  K = 128 is two k-tiles, fewer than the walk drains under; K = 64 is one."""
    M, N = 513, 512
    g = torch.Generator().manual_seed(K)
    x, w, b = _rand(g, M, K), _rand(g, N, K, scale=0.05), _rand(g, N)

    def launch():
        buf, y = _out(M, N)
        hip.linear_drain(x, w, b, y, max_workgroups=1)
        return [buf]
    _both(launch)


@pytest.mark.parametrize("form", ["gated_residual_in_place", "bias"])
def test_workload_k_two_workgroups(hip, form):
    """Nine tiles on two workgroups at the block Linears' K; the gated residual runs in place (res == C) as the engine's does."""
    M, N, K = 600, 768, 3072
    g = torch.Generator().manual_seed(11)
    x, w, b, gate = _rand(g, M, K), _rand(g, N, K, scale=0.02), _rand(g, N), _rand(g, N)
    h0 = _rand(g, M + 3, N + PAD)

    def launch():
        if form == "bias":
            buf, y = _out(M, N)
            hip.linear_drain(x, w, b, y, max_workgroups=2)
        else:
            buf = h0.clone()
            y = buf[:M, :N]
            hip.linear_drain(x, w, b, y, gate0=gate, res0=y, max_workgroups=2)
        return [buf]
    _both(launch)


def test_grouped_two_problems(hip):
    """Tiles of both problems of a grouped launch in one workgroup's list; own A / W / C / gate (and residual) per problem."""
    M0, M1, N, K = 300, 70, 512, 256
    g = torch.Generator().manual_seed(12)
    x0, w0, b0, g0, r0 = _rand(g, M0, K), _rand(g, N, K, scale=0.05), _rand(g, N), _rand(g, N), _rand(g, M0, N + PAD)
    x1, w1, b1, g1, r1 = _rand(g, M1, K), _rand(g, N, K, scale=0.05), _rand(g, N), _rand(g, N), _rand(g, M1, N + PAD)

    def launch():
        buf0, y0 = _out(M0, N)
        buf1, y1 = _out(M1, N)
        hip.linear_drain(x0, w0, b0, y0, x1, w1, b1, y1, gate0=g0, res0=r0[:, :N], gate1=g1, res1=r1[:, :N], max_workgroups=2)
        return [buf0, buf1]
    _both(launch)


def test_split_output_gelu_on_second_part(hip):
    M, N, K, n_split = 300, 768, 256, 256
    g = torch.Generator().manual_seed(13)
    x, w, b = _rand(g, M, K), _rand(g, N, K, scale=0.05), _rand(g, N)

    def launch():
        buf0, y0 = _out(M, n_split)
        buf1, y1 = _out(M, N - n_split)
        hip.linear_drain(x, w, b, y0, y_split=y1, act_split=hip.ACT_GELU_TANH, n_split=n_split, max_workgroups=1)
        return [buf0, buf1]
    _both(launch)


def test_n_not_a_multiple_of_the_tile(hip):
    """N = 328: the second column tile holds 72 columns; chunks past N are dropped, deferred or not."""
    M, N, K = 257, 328, 256
    g = torch.Generator().manual_seed(14)
    x, w, b, r = _rand(g, M, K), _rand(g, N, K, scale=0.05), _rand(g, N), _rand(g, M, N + PAD)

    def launch():
        buf, y = _out(M, N)
        hip.linear_drain(x, w, b, y, res0=r[:, :N], max_workgroups=1)
        return [buf]
    _both(launch)


def test_cap_of_at_least_the_tiles_is_the_one_tile_launch(hip):
    M, N, K = 513, 512, 128
    g = torch.Generator().manual_seed(15)
    x, w, b = _rand(g, M, K), _rand(g, N, K, scale=0.05), _rand(g, N)

    def launch():
        buf, y = _out(M, N)
        hip.linear_drain(x, w, b, y, max_workgroups=6)
        return [buf]
    _both(launch)
