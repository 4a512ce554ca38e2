"""The row-indexed low-rank add (csrc/lora_rows.hip: td_lora_rows_bf16) against its float64 definition (tests/qwen2_lora_common.py), at the smallest shapes
at which it can still go wrong: 1 .. 33 rows (one row, a partial tile, a full tile, a tile and one row, three tiles), ranks 1 / 5 / 16 / 64 (r_pad 16 and 64,
the half-filled last k-step), K of two slabs, six slabs and the 32-slab split, one / two / three output segments into one or two padded buffers."""
import pytest
import torch

import qwen2_lora_common as C

pytestmark = pytest.mark.gpu


def run(hip, case, workspace=None):
    """The kernel on a case: (output buffers on the CPU, the base buffers)."""
    dev = "cuda"
    bufs = [b.to(dev) for b in case["bufs"]]
    packed = [[None if p is None else hip.lora_rows_pack(p[0].to(dev), p[1].to(dev)) for p in per] for per in case["pairs"]]
    ra = torch.tensor(case["row_adapter"], dtype=torch.int32, device=dev)
    hip.lora_rows(case["x"].to(dev), ra, packed, case["ranks"], case["scales"], C.case_views(case, bufs), workspace=workspace)
    torch.cuda.synchronize()
    return [b.cpu() for b in bufs]


def check_untouched(case, out):
    """Rows at -1 (or without a pair for the segment) and the sentinel columns keep their BYTES."""
    refs = C.case_ref(case)
    for s, (got, base) in enumerate(zip(C.case_views(case, out), C.case_views(case, case["bufs"]))):
        keep = ~refs[s][1]
        assert torch.equal(got[keep].view(torch.int16), base[keep].view(torch.int16)), (case["layout"], s)
    mask = [torch.ones_like(b, dtype=torch.bool) for b in out]
    for v in C.case_views(case, mask):
        v[:] = False
    for b, m in enumerate(mask):
        assert torch.equal(out[b][m].view(torch.int16), case["bufs"][b][m].view(torch.int16)), (case["layout"], "sentinel columns of buffer", b)
    return refs


@pytest.mark.parametrize("layout", list(C.LAYOUTS))
def test_exact_integers_are_bit_equal(hip, layout):
    """Every sum is exact whatever the order, so the output equals bf16(float64) bit for bit."""
    cases = [C.make_case(layout, rows, K, (rank, rank), seed=rows * 1000 + rank + K, exact=True) for rows in C.ROWS for rank in C.RANKS for K in C.KS]
    if layout == "three":
        cases.append(C.make_case(layout, 3, C.K_SPLIT, (64, 5), seed=5, exact=True, assignment=[0, 1, -1]))
    for case in cases:
        out = run(hip, case)
        refs = check_untouched(case, out)
        for s, got in enumerate(C.case_views(case, out)):
            y, touched, _ = refs[s]
            assert torch.equal(got[touched].double(), y[touched]), (layout, case["x"].shape, case["ranks"], s)


def test_random_operands_meet_the_bound(hip):
    worst = 0.0
    for case in C.random_cases():
        out = run(hip, case)
        refs = check_untouched(case, out)
        for s, got in enumerate(C.case_views(case, out)):
            y, touched, bound = refs[s]
            err = (got.double() - y).abs()[touched]
            if err.numel():
                ratio = float((err / bound[touched]).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (case["layout"], case["x"].shape, s, ratio)
    print(f"lora_rows: worst error / bound over the random cases: {worst:.3f}")


def test_all_rows_unadapted_changes_nothing(hip):
    case = C.make_case("three", 17, 512, (5, 16), seed=3, assignment=[-1] * 17)
    out = run(hip, case)
    for got, base in zip(out, case["bufs"]):
        assert torch.equal(got.view(torch.int16), base.view(torch.int16))


def test_zero_B_returns_the_base_values(hip):
    case = C.make_case("two", 17, 1536, (16, 5), seed=4, zero_B={0}, assignment=[0] * 9 + [1] * 8)
    out = run(hip, case)
    for got, base in zip(C.case_views(case, out), C.case_views(case, case["bufs"])):
        assert torch.equal(got[:9].float(), base[:9].float())                 # (as values: -0 + 0 is +0)
        assert not torch.equal(got[9:].float(), base[9:].float())


def test_same_call_twice_is_bit_equal(hip):
    """... on the K split too: the slabs are added in a fixed order, no atomics."""
    for case in (C.make_case("three", 3, C.K_SPLIT, (5, 16, 64, 16), seed=1999, null={(1, 0)}, assignment=[0, 2, 3]),
                 C.make_case("two", 33, 1536, (5, 16, 64, 16), seed=7)):
        a, b = run(hip, case), run(hip, case)
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int16), v.view(torch.int16))


def test_a_row_does_not_depend_on_its_neighbours(hip):
    """The K split is a function of K alone: row 5 of a 33-row call carries the bits it has alone."""
    case = C.make_case("one", 33, 1536, (16, 64), seed=11)
    case["row_adapter"][5] = 1
    out = run(hip, case)
    alone = dict(case, x=case["x"][5:6], bufs=[b[5:6].clone() for b in case["bufs"]], row_adapter=[1])
    assert torch.equal(run(hip, alone)[0].view(torch.int16), out[0][5:6].view(torch.int16))


def test_torch_op_gives_what_the_binding_gives(hip):
    from thinkdiff import ops
    T = ops.register()
    case = C.make_case("three", 17, 512, (5, 16, 64, 16), seed=21, null={(1, 0)})
    ref = run(hip, case)
    bufs = [b.cuda() for b in case["bufs"]]
    A, B, pair = [], [], []
    for per in case["pairs"]:
        for p in per:
            pair.append(-1 if p is None else len(A))
            if p is not None:
                A.append(p[0].cuda()); B.append(p[1].cuda())
    T.lora_rows_(case["x"].cuda(), torch.tensor(case["row_adapter"], dtype=torch.int32, device="cuda"), A, B, pair, case["scales"], C.case_views(case, bufs))
    torch.cuda.synchronize()
    for u, v in zip(ref, bufs):
        assert torch.equal(u.view(torch.int16), v.cpu().view(torch.int16))


def test_small_workspace_is_refused(hip):
    case = C.make_case("one", 3, 512, (16,), seed=1)
    with pytest.raises(hip.ThinkDiffHipError, match="ws_bytes"):
        run(hip, case, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
