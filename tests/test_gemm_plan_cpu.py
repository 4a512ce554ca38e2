"""Host-only tile planner (td_gemm_plan_query): alone on the chip it is the lone-launch rule, restated here; under the shared-chip hint of
several images in flight the long-K N = 3072 launches of the FLUX blocks move from the 288x192 to the 256x256 tile, and nothing else moves.
No GPU: the query is arithmetic."""
import os

import pytest

M_GRID = (33, 77, 300, 1024, 1025, 4096, 4289, 4354, 8578)
N_GRID = (64, 72, 1280, 3072, 9216, 12288, 21504)
K_GRID = (3072, 6144, 12288, 15360)
SWITCH = "TD_GEMM_SHARED_TILES"


def lone_rule(M, N, K):
    """The lone-launch rule (csrc/gemm_bf16.hip td_gemm_config_id), K in bf16 equivalents."""
    if N <= 64:
        return 1
    if M <= 32:
        return 2
    t0 = -(-M // 256) * -(-N // 256)
    t3 = -(-M // 288) * -(-N // 192)
    if t0 < 230 and t3 <= 256 and t3 > t0 and K >= 6144 and M > 1024:
        return 3
    return 1 if t0 < 96 else 0


@pytest.fixture
def hip():
    from thinkdiff import _hip
    assert _hip.lib().td_abi_version() >= 19
    prev = os.environ.pop(SWITCH, None)
    yield _hip
    os.environ.pop(SWITCH, None)
    if prev is not None:
        os.environ[SWITCH] = prev


def test_alone_is_the_lone_launch_rule(hip):
    seen = set()
    for M in M_GRID:
        for N in N_GRID:
            for K in K_GRID:
                want = lone_rule(M, N, K)
                seen.add(want)
                assert hip.gemm_plan(M, N, K, shared=False) == want, (M, N, K)
                for op in (hip.OPERAND_INT8, hip.OPERAND_E4M3):      # 8-bit operands: tiles are chosen by bytes
                    assert hip.gemm_plan(M, N, 2 * K, shared=False, operand=op) == want, (M, N, K, op)
                    assert hip.gemm_plan(M, N, K, shared=False, operand=op) == lone_rule(M, N, K // 2), (M, N, K, op)
    assert seen == {0, 1, 3}      # the grid reaches every rule but M <= 32
    assert hip.gemm_plan(32, 3072, 3072) == 2 and hip.gemm_plan(4289, 3072, 15360) == 3 and hip.gemm_plan(4289, 3072, 12288) == 3


def test_shared_chip_takes_the_256x256_tile_for_the_long_k_launches(hip):
    assert hip.gemm_plan(4289, 3072, 15360, shared=True) == 0      # single blocks' proj_out
    assert hip.gemm_plan(4289, 3072, 12288, shared=True) == 0      # double blocks' ff.net.2, image + text rows
    # nothing else moves: a launch the lone rule gives another tile than 288x192 keeps it
    for M in M_GRID:
        for N in N_GRID:
            for K in K_GRID:
                lone = lone_rule(M, N, K)
                got = hip.gemm_plan(M, N, K, shared=True)
                assert got == (lone if lone != 3 else 0), (M, N, K)


def test_shared_chip_keeps_the_small_problem_tiles(hip):
    for K in K_GRID:
        for N in N_GRID:
            for M in (1, 16, 32):
                assert hip.gemm_plan(M, N, K, shared=True) == lone_rule(M, N, K) == (1 if N <= 64 else 2)
        for M in M_GRID:
            for N in (8, 64):
                assert hip.gemm_plan(M, N, K, shared=True) == 1
        assert hip.gemm_plan(300, 3072, K, shared=True) == 1 and hip.gemm_plan(1024, 3072, K, shared=True) == 1      # fewer than 96 tiles


def test_switch_restores_the_lone_launch_rule(hip):
    os.environ[SWITCH] = "0"
    for op in (hip.OPERAND_BF16, hip.OPERAND_INT8, hip.OPERAND_E4M3):
        esz = 1 if op == hip.OPERAND_BF16 else 2
        for M in M_GRID:
            for N in N_GRID:
                for K in K_GRID:
                    assert hip.gemm_plan(M, N, K * esz, shared=True, operand=op) == lone_rule(M, N, K), (op, M, N, K)
    os.environ[SWITCH] = "1"      # ... and 1 forces the CU-time choice for every operand type
    for op in (hip.OPERAND_BF16, hip.OPERAND_INT8, hip.OPERAND_E4M3):
        esz = 1 if op == hip.OPERAND_BF16 else 2
        assert hip.gemm_plan(4289, 3072, 15360 * esz, shared=True, operand=op) == 0
        assert hip.gemm_plan(4289, 3072, 15360 * esz, shared=False, operand=op) == 3      # the switch acts under the hint only


def test_refusals(hip):
    for args in ((0, 3072, 3072, 0, 0), (4289, 0, 3072, 1, 0), (4289, 3072, -64, 1, 0), (4289, 3072, 3072, 1, 3), (4289, 3072, 3072, 0, -1)):
        assert hip.lib().td_gemm_plan_query(*args) == -1
        assert b"td_gemm_plan_query" in hip.lib().td_last_error()
    with pytest.raises(hip.ThinkDiffHipError):
        hip.gemm_plan(4289, 3072, 3072, operand=7)
