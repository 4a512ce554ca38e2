"""Speculative decoding without a GPU: the n-gram proposer, the validation, the generate loop on the stand-in engine (tests/speculative_common.py),
and the refusals of the new C-ABI entries, which arrive before any HIP call."""
import ctypes

import numpy as np
import pytest

import speculative_common as S


@pytest.fixture()
def Q():
    from thinkdiff.models import qwen2_vl
    return qwen2_vl


# ---- ngram_propose ---------------------------------------------------------------------------------------------------------------------------------
def test_ngram_longest_match_wins_over_an_earlier_shorter_one(Q):
    # suffix [5, 6]: the 1-gram [6] occurs first at index 1 (followed by 9), the 2-gram [5, 6] only at index 4 (followed by 7, 8)
    toks = [1, 6, 9, 2, 5, 6, 7, 8, 3, 5, 6]
    assert Q.ngram_propose(toks, 1, 2, 2).tolist() == [7, 8]
    assert Q.ngram_propose(toks, 1, 1, 2).tolist() == [9, 2]


def test_ngram_earliest_occurrence_of_the_winning_length(Q):
    toks = [4, 5, 10, 11, 4, 5, 20, 21, 4, 5]
    assert Q.ngram_propose(toks, 2, 2, 2).tolist() == [10, 11]


def test_ngram_fewer_followers_near_the_end(Q):
    toks = [1, 2, 3, 9, 9, 2, 3]      # [2, 3] at index 1 is followed by 9, 9, 2, 3
    assert Q.ngram_propose(toks, 2, 2, 7).tolist() == [9, 9, 2, 3]
    assert Q.ngram_propose([7, 8, 7], 1, 1, 5).tolist() == [8, 7]


def test_ngram_no_match_and_short_input(Q):
    assert Q.ngram_propose([1, 2, 3, 4], 1, 3, 4).size == 0
    assert Q.ngram_propose([1, 2], 3, 5, 4).size == 0          # n_min > len(tokens)
    assert Q.ngram_propose([], 1, 2, 4).size == 0
    assert Q.ngram_propose([3, 3, 3], 1, 2, 0).size == 0
    out = Q.ngram_propose([3, 3, 3], 1, 2, 4)                   # an overlapping occurrence counts
    assert out.dtype == np.int32 and out.tolist() == [3]


# ---- validation ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("method", "eagle"), ("num_speculative_tokens", 0), ("num_speculative_tokens", 8), ("num_speculative_tokens", True),
                                         ("prompt_lookup_min", 0), ("prompt_lookup_max", 0), ("prompt_lookup_max", 1.5)])
def test_config_validate_names_the_field(Q, field, value):
    kw = dict(method="ngram", num_speculative_tokens=3, prompt_lookup_max=4, prompt_lookup_min=1)
    assert Q.SpeculativeConfig(**kw).validate()
    kw[field] = value
    with pytest.raises(ValueError, match=field):
        Q.SpeculativeConfig(**kw).validate()


def test_vllm_config(Q):
    assert Q.speculative_params_from_vllm_config({}) is None
    c = Q.speculative_params_from_vllm_config({"speculative_config": {"method": "ngram", "num_speculative_tokens": 5, "prompt_lookup_max": 3, "prompt_lookup_min": 2}})
    assert (c.num_speculative_tokens, c.prompt_lookup_max, c.prompt_lookup_min) == (5, 3, 2)
    with pytest.raises(ValueError, match="eagle"):
        Q.speculative_params_from_vllm_config({"speculative_config": {"method": "eagle", "num_speculative_tokens": 2}})
    with pytest.raises(ValueError, match="draft_tensor_parallel_size"):
        Q.speculative_params_from_vllm_config({"speculative_config": {"method": "ngram", "draft_tensor_parallel_size": 1}})
    with pytest.raises(ValueError, match="num_speculative_tokens"):
        Q.speculative_params_from_vllm_config({"speculative_config": {"method": "ngram", "num_speculative_tokens": 9}})
    from thinkdiff.models import mllama_vllm_generate_1, mllama_vllm_t5_embed_decoder_2
    for mod in (mllama_vllm_generate_1, mllama_vllm_t5_embed_decoder_2):
        assert "speculative_params_from_vllm_config" in open(mod.__file__).read()


REFUSED = [("penalty", dict(repetition_penalty=1.2)), ("penalty", dict(presence_penalty=0.5)), ("logit edit", dict(logit_bias={3: 1.0})),
           ("logit edit", dict(allowed_token_ids=[1, 2])), ("logprobs", dict(logprobs=1)), ("n=2", dict(n=2)), ("best_of=2", dict(best_of=2))]


@pytest.mark.parametrize("entry", ["generate", "generate_batch", "generate_continuous"])
@pytest.mark.parametrize("what,extra", REFUSED)
def test_refused_combinations(monkeypatch, entry, what, extra):
    e, Q, ops = S.fake_engine(n_slots=4)
    S.patch(monkeypatch, Q, ops)
    sp = Q.SamplingParams(temperature=0.0, max_tokens=4, min_tokens=1, **extra)
    reqs = S.prompts(2)
    run = {"generate": lambda **kw: e.generate(reqs[0]["prompt_token_ids"], sp, **kw), "generate_batch": lambda **kw: e.generate_batch(reqs, sp, **kw),
           "generate_continuous": lambda **kw: e.generate_continuous(reqs, sp, **kw)}[entry]
    with pytest.raises(ValueError, match=what.split("=")[0]):
        run(speculative=Q.SpeculativeConfig())
    assert e.calls == [], "refused before any engine call"


def test_refused_forced_ids_and_bad_source(monkeypatch):
    e, Q, ops = S.fake_engine(n_slots=4)
    S.patch(monkeypatch, Q, ops)
    sp, reqs = Q.SamplingParams(temperature=0.0, max_tokens=4, min_tokens=1), S.prompts(2)
    with pytest.raises(ValueError, match="forced_output_ids"):
        e.generate_batch(reqs, sp, forced_output_ids=[[1], [2]], speculative=Q.SpeculativeConfig())
    with pytest.raises(ValueError, match="forced_output_ids"):
        e.generate(reqs[0]["prompt_token_ids"], sp, forced_output_ids=[1], speculative=Q.SpeculativeConfig())
    with pytest.raises(ValueError, match="propose"):
        e.generate_continuous(reqs, sp, speculative=object())
    with pytest.raises(ValueError, match="num_speculative_tokens"):
        e.generate_batch(reqs, sp, speculative=Q.SpeculativeConfig(num_speculative_tokens=8))
    assert e.calls == []
    assert not hasattr(Q.Qwen2VLTextEngine.beam_search, "speculative") and "speculative" not in Q.Qwen2VLTextEngine.beam_search.__code__.co_varnames


# ---- the loop on the stand-in engine ---------------------------------------------------------------------------------------------------------------
def _periodic_prompts(n):
    """Prompts that already hold the model's continuation: a chain x, f(x), .., f^15(x), then x again -- prompt lookup finds what follows."""
    out = []
    for i in range(n):
        x, chain = 3 + 11 * i, []
        for _ in range(16):
            chain.append(x)
            x = S.next_token(x)
        out.append({"prompt_token_ids": [50 + i] * (i % 3) + chain + [chain[0]]})
    return out


def _echo(res):
    return [(r["token_ids"], r["hidden_states"][:, 0].float().tolist()) for r in res]


def _run(monkeypatch, entry, reqs, sps_of, draft_of, **ekw):
    e, Q, ops = S.fake_engine(**{**dict(n_slots=8, slot_len=64, prefill_rows=20), **ekw})
    S.patch(monkeypatch, Q, ops)
    kw = {} if draft_of is None else {"speculative": draft_of(Q)}
    if entry == "generate_batch":
        res = e.generate_batch(reqs, sps_of(Q), **kw)
    else:
        res = e.generate_continuous(reqs, sps_of(Q), max_live=3, admit_min=1, **kw)
    return e, res


DRAFTS = {"oracle": lambda Q: S.OracleDraft(), "wrong": lambda Q: S.WrongDraft(),
          "ngram": lambda Q: Q.SpeculativeConfig(num_speculative_tokens=5, prompt_lookup_max=3, prompt_lookup_min=1)}


def _mixed_sampling(Q):
    return [Q.SamplingParams(temperature=0.0 if i % 2 == 0 else 1.0, seed=None if i % 2 == 0 else 40 + i, max_tokens=5 + 3 * i, min_tokens=1) for i in range(5)]


@pytest.mark.parametrize("entry", ["generate_batch", "generate_continuous"])
@pytest.mark.parametrize("draft", sorted(DRAFTS))
def test_loop_returns_the_plain_run(monkeypatch, entry, draft):
    """Tokens and hidden echoes of the non-speculative run, exactly; the acceptance each draft source must show; no fed row past a slot's capacity
    (the stand-in asserts it) or a request's budget (asserted from the logged calls)."""
    reqs = _periodic_prompts(5)
    _, plain = _run(monkeypatch, entry, reqs, _mixed_sampling, None)
    e, spec = _run(monkeypatch, entry, reqs, _mixed_sampling, DRAFTS[draft])
    assert _echo(spec) == _echo(plain)
    for i, r in enumerate(spec):
        assert len(r["token_ids"]) == 5 + 3 * i == r["hidden_states"].shape[0]
    st = e.spec_stats()
    assert st["emitted"] == sum(len(r["token_ids"]) for r in spec) and st["steps"] > 0
    if draft == "oracle":      # greedy rows accept every guess; the seeded rows' shifted draws reject theirs
        assert st["accepted"] > 0 and st["steps"] < max(len(r["token_ids"]) for r in plain)
    elif draft == "wrong":
        assert st["drafted"] > 0 and st["accepted"] == 0
    else:
        assert st["accepted"] > 0
    # budgets: a sequence never feeds more rows than it may still emit
    verifies = [c for c in e.calls if c[0] == "verify"]
    assert verifies and all(max(c[2]) <= 8 and sum(c[2]) <= 256 for c in verifies)


def test_oracle_draft_accepts_everything_and_saves_steps(monkeypatch):
    reqs = _periodic_prompts(4)
    sps = lambda Q: Q.SamplingParams(temperature=0.0, max_tokens=24, min_tokens=24)
    _, plain = _run(monkeypatch, "generate_batch", reqs, sps, None)
    e, spec = _run(monkeypatch, "generate_batch", reqs, sps, DRAFTS["oracle"])
    assert _echo(spec) == _echo(plain)
    st = e.spec_stats()
    assert st["accepted"] == st["drafted"] > 0 and st["emitted"] == 4 * 24
    assert st["steps"] == 3, "24 tokens at 8 rows per step"
    # the budget cap from the logged calls: cache_pos + n_new never passes prompt + max_tokens
    lens = {i: len(r["prompt_token_ids"]) for i, r in enumerate(reqs)}
    for slot, pos, n_new in e.verify_rows:
        assert pos + n_new <= lens[slot] + 24


def test_budget_and_capacity_caps_from_the_logged_calls(monkeypatch):
    """Odd budgets and a slot that fills up: every verify row stays inside min(prompt + max_tokens, slot_len)."""
    reqs = _periodic_prompts(3)
    sps = lambda Q: [Q.SamplingParams(temperature=0.0, max_tokens=m, min_tokens=1) for m in (1, 10, 30)]
    _, plain = _run(monkeypatch, "generate_batch", reqs, sps, None, slot_len=32)
    e, spec = _run(monkeypatch, "generate_batch", reqs, sps, DRAFTS["oracle"], slot_len=32)
    assert _echo(spec) == _echo(plain)
    assert len(spec[2]["token_ids"]) < 30, "the third sequence retires when its slot is full"
    lens = [len(r["prompt_token_ids"]) for r in reqs]
    assert e.verify_rows
    for slot, pos, n_new in e.verify_rows:
        assert pos + n_new <= min(lens[slot] + (1, 10, 30)[slot], 32)


def test_stop_id_inside_an_accepted_run_cuts_there(monkeypatch):
    reqs = _periodic_prompts(2)
    chain = reqs[0]["prompt_token_ids"]
    stop = chain[4]      # the 4th generated token of request 0 (generation restarts the chain at chain[1])
    sps = lambda Q: Q.SamplingParams(temperature=0.0, max_tokens=20, min_tokens=2, stop_token_ids=[stop])
    _, plain = _run(monkeypatch, "generate_batch", reqs, sps, None)
    e, spec = _run(monkeypatch, "generate_batch", reqs, sps, DRAFTS["oracle"])
    assert _echo(spec) == _echo(plain)
    assert spec[0]["token_ids"][-1] == stop and len(spec[0]["token_ids"]) == 4 and len(spec[1]["token_ids"]) == 20
    first = next(c for c in e.calls if c[0] == "verify")
    assert first[2][0] == 8, "the stop id sat inside a run of 8 fed rows"


def test_step_without_drafts_is_a_plain_decode_call(monkeypatch):
    reqs = S.prompts(3)      # random prompts: nothing for prompt lookup to find at first
    sps = lambda Q: Q.SamplingParams(temperature=0.0, max_tokens=3, min_tokens=3)
    _, plain = _run(monkeypatch, "generate_batch", reqs, sps, None, prefill_rows=8)
    e, spec = _run(monkeypatch, "generate_batch", reqs, sps, lambda Q: Q.SpeculativeConfig(num_speculative_tokens=2, prompt_lookup_max=6, prompt_lookup_min=6), prefill_rows=8)
    assert _echo(spec) == _echo(plain)
    kinds = [c[0] for c in e.calls]
    assert "verify" not in kinds and kinds.count("decode") == 3
    assert e.spec_stats() == dict(steps=3, drafted=0, accepted=0, emitted=9)


def test_generate_takes_the_batch_path(monkeypatch):
    e, Q, ops = S.fake_engine(n_slots=2)
    S.patch(monkeypatch, Q, ops)
    p = _periodic_prompts(1)[0]["prompt_token_ids"]
    sp = Q.SamplingParams(temperature=0.0, max_tokens=12, min_tokens=12)
    spec = e.generate(p, sp, speculative=S.OracleDraft())
    e2, Q2, ops2 = S.fake_engine(n_slots=2)
    S.patch(monkeypatch, Q2, ops2)
    plain = e2.generate(p, sp)
    assert spec["token_ids"] == plain["token_ids"] and spec["hidden_states"][:, 0].tolist() == plain["hidden_states"][:, 0].tolist()
    assert e.spec_stats()["accepted"] == e.spec_stats()["drafted"] == 10      # 7 guesses, then 12 - 8 - 1 = 3


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from thinkdiff import _hip
    return _hip.lib()


def _refused(L, rc, *words):
    msg = L.td_last_error().decode()
    assert rc == 2, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_abi_version(L):
    assert L.td_abi_version() >= 21


def test_attention_verify_refusals_before_any_hip_call(L):
    """Host-only arguments: the pointers are never dereferenced, every call returns TD_ERR_INVALID from the argument checks."""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    p = ctypes.c_void_p
    ok = dict(q=p(a), ldq=1536, k=p(a), v=p(a), ldkv=512, kvb=512 * 64, k8=None, v8=None, ks=None, vs=None, lds=0, sb=0, o=p(a), ldo=1536, n=3,
              r0=p(a), rows=p(a), len0=p(a), slot=p(a), Hq=12, Hkv=2)

    def call(**kw):
        d = {**ok, **kw}
        return L.td_attention_verify(d["q"], d["ldq"], d["k"], d["v"], d["ldkv"], d["kvb"], d["k8"], d["v8"], d["ks"], d["vs"], d["lds"], d["sb"], d["o"], d["ldo"],
                                     d["n"], d["r0"], d["rows"], d["len0"], d["slot"], d["Hq"], d["Hkv"], 0.088, None)
    _refused(L, call(q=None), "null q")
    _refused(L, call(o=None), "null q")
    _refused(L, call(rows=None), "per-sequence")
    _refused(L, call(k=None, v=None), "exactly one cache form")
    _refused(L, call(k8=p(a), v8=p(a), ks=p(a), vs=p(a)), "exactly one cache form")
    _refused(L, call(k=None, v=None, k8=p(a), v8=p(a), ks=p(a), vs=None, lds=4), "both scale planes")
    _refused(L, call(v=None), "bf16 form")
    _refused(L, call(n=0), "n_seq=0")
    _refused(L, call(n=257), "n_seq=257")
    _refused(L, call(Hq=13), "Hq=13")
    _refused(L, call(ldq=1532), "ldq=1532")
    _refused(L, call(ldkv=250), "ldkv=250")
    _refused(L, call(q=p(a + 8)), "16-byte")
    _refused(L, call(k=p(a + 8)), "16-byte")
    _refused(L, call(k=None, v=None, k8=p(a + 4), v8=p(a), ks=p(a), vs=p(a), lds=4), "8-byte")
    prev = L.td_attention_verify_set_form(2)
    assert L.td_attention_verify_set_form(prev) == 2


def test_spec_accept_refusals_before_any_hip_call(L):
    buf = (ctypes.c_char * 256)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    p = ctypes.c_void_p
    _refused(L, L.td_spec_accept(None, p(a), p(a), p(a), 1, p(a), p(a), None), "null input")
    _refused(L, L.td_spec_accept(p(a), p(a), p(a), p(a), 1, None, p(a), None), "null output")
    _refused(L, L.td_spec_accept(p(a), p(a), p(a), p(a), 0, p(a), p(a), None), "B=0")
    _refused(L, L.td_spec_accept(p(a), p(a), p(a), p(a), 257, p(a), p(a), None), "B=257")
    _refused(L, L.td_spec_accept(p(a + 2), p(a), p(a), p(a), 1, p(a), p(a), None), "4-byte")


def test_verify_batch_refusals_before_any_launch(L):
    """td_qwen2_verify_batch_slots on a NULL handle or NULL arrays: refused by the first check, nothing is dereferenced."""
    buf = (ctypes.c_int * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    _refused(L, L.td_qwen2_verify_batch_slots(None, 1, None, p, p, p, p, None, None, None), "td_qwen2_verify_batch", "null")
    _refused(L, L.td_qwen2_verify_batch_slots(p, 1, None, None, p, p, p, None, None, None), "td_qwen2_verify_batch", "null")
