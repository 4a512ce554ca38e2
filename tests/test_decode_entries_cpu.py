"""The decode entries of Qwen2VLTextEngine -- generate, generate_batch, generate_continuous, beam_search -- call for call on the stand-in engines:

  * tests/golden/decode_entries_calls.json holds the stand-in's call log and the results of parallel_sampling_common.entry_scenarios, recorded at the
    commit BEFORE the three generate loops were folded onto one token source, one prompt prefill and one live-row table; the replay must equal it
    entry for entry (the stand-in logs a decode step the same whether it arrives through decode_batch or _decode_slots);
  * generate_batch and beam_search with packed_prefill on, which only the shared _prefill_prompts lets a stand-in reach: where the passes are cut,
    which slots they fill, and the same tokens, hidden echoes and outputs as one forward per prompt."""
import json
import os

import torch

import beam_search_common as B
import parallel_sampling_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_entry_makes_the_calls_of_the_commit_before(monkeypatch):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "decode_entries_calls.json")))
    from thinkdiff.models import qwen2_vl as Q
    monkeypatch.setattr(Q.Qwen2VLTextEngine, "_draw_sampler_key", staticmethod(lambda generator=None: C.KEY))
    got = C.run_entries_trace(lambda Q, ops: monkeypatch.setattr(Q, "_OPS", ops))
    assert sorted(got) == sorted(golden) and len(got) == 23
    for name in golden:
        assert got[name]["calls"] == golden[name]["calls"], name
        assert got[name]["results"] == golden[name]["results"], name


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["token_ids"] == y["token_ids"]
        assert torch.equal(x["hidden_states"], y["hidden_states"]) and torch.equal(x["prompt_hidden_states"], y["prompt_hidden_states"])
        assert ("outputs" in x) == ("outputs" in y)
        for o, p in zip(x.get("outputs", []), y.get("outputs", [])):
            assert o["index"] == p["index"] and o["token_ids"] == p["token_ids"] and torch.equal(o["hidden_states"], p["hidden_states"])
            assert o.get("cumulative_logprob") == p.get("cumulative_logprob")


def test_generate_batch_packs_its_prompts_into_passes_cut_at_prefill_rows(monkeypatch):
    reqs = C.prompts(7)      # 1, 4, 7, 2, 5, 8, 3 tokens
    lens = [len(r["prompt_token_ids"]) for r in reqs]
    assert lens == [1, 4, 7, 2, 5, 8, 3]

    def run(packed):
        # (unpacked: a prefill_rows below two padded prompts, so that the stand-in, which has no padded prefill, gets one forward per prompt)
        e, Q, ops = C.fake_engine(n_slots=12, slot_len=32, prefill_rows=16 if packed else 8)
        C.patch(monkeypatch, Q, ops)
        e.packed_prefill = packed
        sps = [Q.SamplingParams(temperature=1.0, seed=50 + i, max_tokens=2 + i % 3, min_tokens=1, n=(1, 3, 1, 1, 2, 1, 1)[i], best_of=3 if i == 4 else None)
               for i in range(7)]
        return e, e.generate_batch(reqs, sps)

    e, res = run(True)
    pre = [c for c in e.calls if c[0] in ("prefill", "forward")]
    assert pre == [["prefill", [0, 1, 2, 3], [1, 4, 7, 2]], ["prefill", [4, 5, 6], [5, 8, 3]]]      # 14 of 16 rows (5 more do not fit), then exactly 16
    assert all(sum(c[2]) <= 16 for c in pre) and [s for c in pre for s in c[1]] == list(range(7)), "slots 0 .. B-1 in request order"
    kinds = [c[0] for c in e.calls]
    assert max(i for i, k in enumerate(kinds) if k == "prefill") < min(i for i, k in enumerate(kinds) if k == "fork"), "forks come after all prefills"
    assert [c[1:] for c in e.calls if c[0] == "fork"] == [[1, [7, 8], 4], [4, [9, 10], 5]], "children take the slots from B up"
    e2, res2 = run(False)
    assert [c for c in e2.calls if c[0] in ("prefill", "forward")] == [["forward", b, n] for b, n in enumerate(lens)]
    assert [c for c in e.calls if c[0] not in ("prefill", "forward")] == [c for c in e2.calls if c[0] not in ("prefill", "forward")]
    _same_results(res, res2)
    assert [len(r.get("outputs", [])) for r in res] == [0, 3, 0, 0, 2, 0, 0]


def test_beam_search_packs_its_prompts_and_takes_one_forward_each_without(monkeypatch):
    prompts = [[1, 2, 3], [4, 5, 6, 7, 0, 9, 10], [8], [11, 0, 2, 5, 6, 1, 3, 9]]

    def run(packed):
        e, Q, ops = B.fake_engine(n_slots=8, slot_len=32, prefill_rows=16)
        monkeypatch.setattr(Q, "_OPS", ops)
        e.packed_prefill = packed
        return e, e.beam_search([{"prompt_token_ids": p} for p in prompts], Q.BeamSearchParams(beam_width=2, max_tokens=4), eos_token_id=3)

    e, res = run(True)
    pre = [c for c in e.calls if c[0] in ("prefill", "forward")]
    assert pre == [["prefill", [0, 2, 4], [3, 7, 1]], ["prefill", [6], [8]]], "11 rows of 16, then the prompt that no longer fits; each request's first slot"
    e2, res2 = run(False)
    assert [c for c in e2.calls if c[0] in ("prefill", "forward")] == [["forward", 2 * r, len(p)] for r, p in enumerate(prompts)]
    assert [c for c in e.calls if c[0] not in ("prefill", "forward")] == [c for c in e2.calls if c[0] not in ("prefill", "forward")]
    _same_results(res, res2)
    for x, y in zip(res, res2):
        assert [o["score"] for o in x["outputs"]] == [o["score"] for o in y["outputs"]]
