"""The operands of tests/test_attention_prefix_gpu.py are decisive: in float64, every masking / indexing mutant of the context-attention reference lies
at least 10x that test's bar (2^-7 max|ref| per segment) from the true output, on every segment the mutant concerns
(tests/attention_prefix_cases_common.py says which and why).  No GPU."""
import pytest
import torch

import attention_prefix_cases_common as P

MUTANTS = ["causal offset + 1", "causal offset - 1", "first key dropped", "prefix dropped", "neighbouring slot visible", "row0 of the segment in front",
           "offset from the longest"]


def test_the_cases_are_the_ones_the_kernel_can_go_wrong_at():
    assert P.CASES == [(1, 0), (1, 1), (1, 63), (1, 64), (2, 300), (31, 1), (32, 32), (33, 255), (64, 64), (65, 191), (255, 1), (256, 256), (257, 63),
                       (300, 513), (16, 1040)]
    assert P.HEADS == [(4, 2), (7, 1)]
    assert P.SLOT_ROWS == 1400 and max(n + p for n, p in P.CASES) <= P.SLOT_ROWS
    for Hq, Hkv in P.HEADS:      # no used slot starts at a multiple of the key tile
        assert all((s * P.SLOT_ROWS) % 64 for s in P.slots_of(Hq, Hkv))


@pytest.mark.parametrize("Hq,Hkv", P.HEADS)
def test_layout_of_the_operands(Hq, Hkv):
    case = P.prefix_case(Hq, Hkv)
    slots = case["slots"]
    assert len(set(slots)) == len(P.CASES) and 0 not in slots and slots != sorted(slots), "slots distinct, scrambled, slot 0 unused"
    assert P.slots_of(4, 2) != P.slots_of(7, 1)
    assert case["row0"].tolist() == [s * P.SLOT_ROWS for s in slots] and case["kv_lens"].tolist() == [n + p for n, p in P.CASES]
    KW = Hkv * P.D
    cache, pad = case["cache"].float(), float(torch.tensor(P.PAD).bfloat16())      # (1e4 as bf16 holds it)
    inside = torch.zeros(cache.shape[0], dtype=torch.bool)
    for b, (n, p) in enumerate(P.CASES):
        inside[slots[b] * P.SLOT_ROWS:slots[b] * P.SLOT_ROWS + n + p] = True
    assert (cache[~inside] == pad).all(), "a row outside every segment's key range does not hold 1e4"
    assert (cache[:, 2 * KW:] == pad).all() and (case["qbuf"][:, Hq * P.D:].float() == pad).all(), "pad columns"
    assert cache[inside][:, :2 * KW].abs().max() < 100
    assert torch.isfinite(case["ref"]).all() and case["ref"].shape == (sum(n for n, _ in P.CASES), Hq * P.D)
    for n, p in P.CASES:      # no key is owned by two rows
        succ, diag, first = P.plants(n, p)
        keys = [p + r + 1 for r in succ] + [p + r for r in diag] + ([0] if first is not None and p + n - 1 != 0 else [])
        assert len(set(keys)) == len(keys) and max(keys) <= n + p - 1


@pytest.mark.parametrize("Hq,Hkv", P.HEADS)
def test_every_mutant_is_far_from_the_reference(Hq, Hkv):
    case = P.prefix_case(Hq, Hkv)
    margins = P.prefix_margins(case)
    assert sorted(margins) == sorted(MUTANTS)
    n = len(P.CASES)
    longest = max(q for q, _ in P.CASES)
    concerned = {"causal offset + 1": n, "causal offset - 1": n - 1, "first key dropped": n - 1, "prefix dropped": sum(p >= 1 for _, p in P.CASES),
                 "neighbouring slot visible": n, "row0 of the segment in front": n - 1, "offset from the longest": sum(q < longest for q, _ in P.CASES)}
    for name in MUTANTS:
        assert len(margins[name]) == concerned[name], name
        what, worst = min(margins[name], key=lambda x: x[1])
        print(f"Hq={Hq} Hkv={Hkv} {name}: smallest margin {worst:.1f} x the bar ({what})")
        assert worst >= P.MIN_MARGIN, f"{name}: only {worst:.2f} x the bar at {what}"
