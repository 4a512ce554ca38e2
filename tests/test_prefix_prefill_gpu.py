"""The packed prefill behind cached prefixes (td_qwen2_prefill_packed_prefix_slots) against the full packed prefill and against one forward per sequence.

Tiny engines as in tests/test_spec_decode_gpu.py (2 layers, both decoder widths, scaled weights), modes bf16, kv_fp8 (the staged path over the e4m3 cache)
and w_fp8.  Bound between two schedules of one model: the project's _rel < 5e-3.

Measured on MI355X, worst _rel over hidden rows, logits and new cache rows, against both references: 2.6e-3 .. 3.1e-3 over the six (width, mode) cases."""
import ctypes

import pytest
import torch

from test_spec_decode_gpu import SHAPES, VOCAB, _rel, _weights

pytestmark = pytest.mark.gpu

MODES = {"bf16": {}, "kv_fp8": dict(kv="fp8"), "w_fp8": dict(quant="fp8")}
PREFIX = [0, 16, 48, 33, 96]
NEW = [20, 7, 30, 1, 25]
SLOTS = [4, 0, 6, 1, 3]
ALONE = [8, 9, 10, 11, 12]      # slots of the one-sequence-at-a-time reference, on the same engine


def _engine(shape, mode, max_len=128, slots=16, seed=7, prefill_rows=None):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    m = MODES[mode]
    cfg = Qwen2VLTextConfig(num_hidden_layers=2, intermediate_size=2048, vocab_size=VOCAB, **SHAPES[shape])
    e = Qwen2VLTextEngine(cfg, max_model_len=max_len, n_slots=slots, kv_cache_dtype=m.get("kv", "auto"), prefill_rows=prefill_rows)
    e.load_state_dict(_weights(shape, seed))
    if m.get("quant"):
        e.quantize_weights(m["quant"])
    return e


def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, VOCAB, (p + n,), generator=g, dtype=torch.int32) for p, n in zip(PREFIX, NEW)]


def _rows(e, toks, a=0):
    return {"token_ids": toks[a:], "position_ids": e.text_position_ids(len(toks))[:, a:]}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_prefix_prefill_against_the_full_prefill(hip, shape, mode):
    """Engine A prefills 5 prompts in full.  Engine B gets the first PREFIX = [0, 16, 48, 33, 96] rows of each by forward, then the rest through
    prefill_packed with those prefixes, slots [4, 0, 6, 1, 3].  Per sequence _rel < 5e-3 on the hidden rows, the last token's logits and the new cache rows
    of both layers; the prefix rows of the cache are bit-unchanged; the same bound against forward(pos0 = prefix) one sequence at a time."""
    prompts = _prompts()
    A, B = _engine(shape, mode, prefill_rows=512), _engine(shape, mode, prefill_rows=512)
    hid_a, lg_a = A.prefill_packed([_rows(A, t) for t in prompts], SLOTS, [0] * 5)
    for t, p, s, s2 in zip(prompts, PREFIX, SLOTS, ALONE):
        if p:
            B.forward(B.text_position_ids(len(t))[:, :p], t[:p], slot=s, want_hidden=False)
            B.forward(B.text_position_ids(len(t))[:, :p], t[:p], slot=s2, want_hidden=False)
    before = [[B.read_kv(l, s, 0, p).clone() if p else None for l in range(2)] for s, p in zip(SLOTS, PREFIX)]
    hid_b, lg_b = B.prefill_packed([_rows(B, t, p) for t, p in zip(prompts, PREFIX)], SLOTS, PREFIX)
    torch.cuda.synchronize()
    worst = 0.0
    for b, (t, p, n, s, s2) in enumerate(zip(prompts, PREFIX, NEW, SLOTS, ALONE)):
        assert hid_b[b].shape == (n, A.config.hidden_size)
        eh, el = _rel(hid_b[b], hid_a[b][p:]), _rel(lg_b[b], lg_a[b])
        assert eh < 5e-3 and el < 5e-3, f"sequence {b} (prefix {p}, {n} new rows): hidden {eh:.2e}, logits {el:.2e}"
        worst = max(worst, eh, el)
        for layer in range(2):
            ek = _rel(B.read_kv(layer, s, p, n), A.read_kv(layer, s, p, n))
            assert ek < 5e-3, f"sequence {b}, layer {layer}: new cache rows {ek:.2e}"
            worst = max(worst, ek)
            if p:
                assert torch.equal(B.read_kv(layer, s, 0, p), before[b][layer]), f"sequence {b}, layer {layer}: the prefix rows of the cache changed"
        # one sequence at a time: forward at pos0 = prefix behind the same prefix rows
        h1, l1 = B.forward(B.text_position_ids(len(t))[:, p:], t[p:], pos0=p, want_logits=True, slot=s2)
        e1, e2 = _rel(hid_b[b], h1), _rel(lg_b[b], l1)
        assert e1 < 5e-3 and e2 < 5e-3, f"sequence {b} against forward(pos0={p}): hidden {e1:.2e}, logits {e2:.2e}"
        worst = max(worst, e1, e2)
    print(f"prefix prefill {shape} {mode}: worst _rel {worst:.2e} (bound 5e-3)")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_all_prefixes_zero_is_the_packed_prefill(hip, mode):
    """Every prefix 0: the call delegates to td_qwen2_prefill_packed_slots -- the same bits."""
    prompts = _prompts()
    e = _engine("2b", mode, prefill_rows=512)
    hid_a, lg_a = e.prefill_packed([_rows(e, t) for t in prompts], SLOTS, [0] * 5)
    emb, pos, lens = e._pack_prompts([{"prompt_token_ids": t.tolist()} for t in prompts], [e.text_position_ids(len(t)) for t in prompts])
    hid = torch.empty(sum(lens), e.config.hidden_size, dtype=torch.bfloat16, device="cuda")
    lg = torch.empty(5, VOCAB, dtype=torch.bfloat16, device="cuda")
    e._prefill_packed_slots(5, (ctypes.c_int * 5)(*SLOTS), emb, pos, (ctypes.c_int * 5)(*lens), hid, lg)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(hid_a), hid) and torch.equal(lg_a, lg)


def test_refusals_name_the_value(hip):
    e = _engine("2b", "kv_fp8", max_len=128, slots=4)      # 4 slots of 128 rows, a workspace of 128 rows
    rows = lambda n: {"token_ids": torch.zeros(n, dtype=torch.int32), "position_ids": e.text_position_ids(n)}

    def refused(word, reqs, slots, prefixes):
        with pytest.raises(hip.ThinkDiffHipError, match=word):
            e.prefill_packed(reqs, slots, prefixes)

    # the e4m3 cache stages prefix + new rows: 3 x (48 + 8) = 168 > 128 workspace rows, though the 24 new rows fit
    refused("168 staged rows exceed the 128 workspace rows", [rows(8)] * 3, [0, 1, 2], [48, 48, 48])
    refused("names cache slot 4 of 4", [rows(8)], [4], [16])
    refused("cache slot 1 is named by more than one", [rows(8)] * 2, [1, 1], [16, 0])
    refused("prefix_lens=-16", [rows(8)], [0], [-16])
    refused("prefix 124 \\+ 8 new rows exceed the slot capacity 128", [rows(8)], [0], [124])
    refused("136 packed rows exceed the 128 workspace rows", [rows(68)] * 2, [0, 1], [16, 0])
    L, c = hip.lib(), ctypes
    one = (c.c_int * 1)(0)
    z = torch.zeros(8, e.config.hidden_size, dtype=torch.bfloat16, device="cuda")
    pos = e.text_position_ids(8).to("cuda").contiguous()
    for B, lens, word in ((0, [8], b"0 sequences"), (257, [8], b"257 sequences"), (1, [0], b"lens=0")):
        rc = L.td_qwen2_prefill_packed_prefix_slots(e._h, B, c.cast(one, c.c_void_p), None, hip.ptr(z), hip.ptr(pos), c.cast((c.c_int * 1)(*lens), c.c_void_p),
                                                   c.cast((c.c_int * 1)(16), c.c_void_p), None, None, hip.stream_ptr())
        assert rc == 2 and word in L.td_last_error(), (B, lens, L.td_last_error())
