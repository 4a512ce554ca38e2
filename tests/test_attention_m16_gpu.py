"""The score-bound joint attention on the 16x16x32 MFMA body against the 32x32x16 body it replaces, both against fp64.

Reference: softmax_2(q . k^T) . v in float64 on the CPU from the bf16 inputs (q arrives pre-scaled, so the scores are in log2 units).
Inputs: q and k uniform in +-0.25, so |s| <= 128 x 0.0625 = 8 octaves = the score bound handed over; v from N(0, 1).

Both bodies round at the same points (probabilities to bf16 before P.V, row sums over the rounded values, the output to bf16) and differ in the
order of the fp32 sums only, so their errors against fp64 are statistically equal.  The bar is therefore measured, not typed in: per shape the
new body's RMS and max-abs error must be no worse than 1.25 x the 32x32x16 body's on the same inputs (the margin covers sample variation on
the small shapes).  Both errors of every shape are recorded in profiles/attention_m16_parity.json.

Shapes.  One workgroup per item: (64, 1) one tile; (65, 1) a ragged second KV tile and a ragged q block; (257, 3) a second q tile with one live
row; (321, 2).  Persistent form: (257, 160) = 320 items on 256 CUs, 5 KV tiles per item and ranges of 6.25 tiles, so every range crosses an item
boundary and every hand-off path runs; it launches on a stream of its own, i.e. with a hand-off workspace of its own, zero-filled when created.
The output buffer is one row longer than S and pre-filled with a sentinel: the extra row must stay untouched."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCE_32 = 0x400      # td_attention_set_variant bit: the 32x32x16 body
SENTINEL = -12352.0      # (a bf16 value)
BOUND = 8.0


def _record(key, value):
    fn = os.path.join(ROOT, "profiles", "attention_m16_parity.json")
    data = json.load(open(fn)) if os.path.exists(fn) else {}
    data[key] = value
    with open(fn, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


def _case(S, H):
    g = torch.Generator().manual_seed(1000 * S + H)
    W = H * 128
    qkv = torch.empty(S, 3 * W)
    qkv[:, :2 * W] = torch.rand(S, 2 * W, generator=g) * 0.5 - 0.25
    qkv[:, 2 * W:] = torch.randn(S, W, generator=g)
    qkv = qkv.bfloat16()
    x = qkv.double().view(S, 3, H, 128)
    s = torch.einsum("qhd,khd->hqk", x[:, 0], x[:, 1])
    assert float(s.abs().max()) <= BOUND
    p = torch.exp2(s)
    ref = torch.einsum("hqk,khd->qhd", p / p.sum(-1, keepdim=True), x[:, 2]).reshape(S, W)
    return qkv, ref


def _run(hip, qkv, S, H, variant):
    W = H * 128
    d = qkv.cuda()
    out = torch.full((S + 1, W), SENTINEL, dtype=torch.bfloat16, device="cuda")
    prev = hip.lib().td_attention_set_variant(variant)
    try:
        hip.attention_joint_prescaled(d[:, :W], d[:, W:2 * W], d[:, 2 * W:], out[:S], H, BOUND)
        torch.cuda.synchronize()
    finally:
        hip.lib().td_attention_set_variant(prev)
    o = out.float().cpu()
    assert bool((o[S] == SENTINEL).all()), "the row behind the last query row was written"
    assert torch.isfinite(o[:S]).all() and not bool((o[:S] == SENTINEL).any()), "an output element was not written"
    return o[:S].double()


def _compare(hip, S, H, form):
    qkv, ref = _case(S, H)
    err = {}
    for name, variant in (("m32", FORCE_32), ("m16", 0)):
        e = _run(hip, qkv, S, H, variant) - ref
        err[name] = {"rms": float(e.pow(2).mean().sqrt()), "max_abs": float(e.abs().max())}
    print(f"{form} S={S} H={H}: 32x32x16 rms {err['m32']['rms']:.4e} max {err['m32']['max_abs']:.4e} | 16x16x32 rms {err['m16']['rms']:.4e} max {err['m16']['max_abs']:.4e}")
    _record(f"{form}_S{S}_H{H}", err)
    assert err["m32"]["rms"] > 0.0
    assert err["m16"]["rms"] <= 1.25 * err["m32"]["rms"]
    assert err["m16"]["max_abs"] <= 1.25 * err["m32"]["max_abs"]


@pytest.mark.parametrize("S,H", [(64, 1), (65, 1), (257, 3), (321, 2)])
def test_m16_body_one_workgroup_per_item(hip, S, H):
    _compare(hip, S, H, "lean")


def test_m16_body_persistent_with_handoffs(hip):
    S, H = 257, 160
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-S // 256) * H > cus, "the shape must exceed one round of workgroups to take the persistent form"
    with torch.cuda.stream(torch.cuda.Stream()):
        _compare(hip, S, H, "streamk")
