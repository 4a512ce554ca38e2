"""Logit edits and logprobs without a GPU: the new SamplingParams fields, the C ABI's argument errors, the op schemas, the ban planner against a
brute-force restatement of vLLM's bad-words and min-tokens rules (tests/logit_edits_common.py), the routing of a request with an edit through
sample_rows_edit (a stand-in engine) and the vllm_config pass-through of the two model classes."""
import ctypes
import importlib
import os
import random
from types import SimpleNamespace

import pytest
import torch

import logit_edits_common as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
TD_ERR_INVALID = 2


# ---- SamplingParams ----------------------------------------------------------------------------------------------------
def test_defaults_are_off_and_keep_the_old_route():
    from thinkdiff.models.qwen2_vl import SamplingParams
    sp = SamplingParams()
    assert (sp.logit_bias, sp.allowed_token_ids, sp.bad_words_token_ids, sp.mask_stop_below_min_tokens, sp.logprobs) == (None, None, None, False, None)
    assert sp.validate() is sp and not sp.per_request and not sp.has_edit
    assert not SamplingParams(logprobs=5).validate().per_request, "logprobs alone does not change which sampler runs"
    assert not SamplingParams(mask_stop_below_min_tokens=True).has_edit, "the reference's defaults (ignore_eos, no stop ids) mask nothing"
    assert not SamplingParams(mask_stop_below_min_tokens=True, stop_token_ids=[3], min_tokens=0).has_edit
    for kw in (dict(logit_bias={3: 1.5}), dict(allowed_token_ids=[1, 2]), dict(bad_words_token_ids=[[4]]),
               dict(mask_stop_below_min_tokens=True, stop_token_ids=[3]), dict(mask_stop_below_min_tokens=True, ignore_eos=False)):
        sp = SamplingParams(**kw).validate()
        assert sp.has_edit and sp.per_request and not sp.has_penalty, kw


@pytest.mark.parametrize("field,value", [("logit_bias", {-1: 1.0}), ("logit_bias", {3: float("inf")}), ("logit_bias", {3: float("nan")}), ("logit_bias", {1.5: 1.0}),
                                         ("logit_bias", [1, 2]), ("logit_bias", {i: 0.5 for i in range(1025)}), ("allowed_token_ids", []),
                                         ("allowed_token_ids", [1, -2]), ("allowed_token_ids", "12"), ("bad_words_token_ids", [[]]), ("bad_words_token_ids", [[1, -1]]),
                                         ("bad_words_token_ids", ["ab"]), ("bad_words_token_ids", [3]), ("mask_stop_below_min_tokens", 1), ("logprobs", -1),
                                         ("logprobs", 21), ("logprobs", 2.5), ("logprobs", True)])
def test_validate_names_the_field_and_value(field, value):
    from thinkdiff.models.qwen2_vl import SamplingParams
    with pytest.raises(ValueError) as e:
        SamplingParams(**{field: value}).validate()
    assert f"SamplingParams.{field}=" in str(e.value) and repr(value) in str(e.value)


def test_limits_are_accepted():
    from thinkdiff.models.qwen2_vl import SamplingParams
    SamplingParams(logit_bias={i: -100.0 for i in range(1024)}, logprobs=20, allowed_token_ids=[0], bad_words_token_ids=[[1], [2, 3, 4]]).validate()
    SamplingParams(logprobs=0).validate()


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def _lib():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    lib.td_sample_row_size.restype = ctypes.c_size_t
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.td_logit_edits_create.argtypes = [i32, i32, vp]
    lib.td_logit_edits_reset_slot.argtypes = [vp, i32, vp]
    lib.td_logit_edits_set_bias.argtypes = [vp, i32, vp, vp, i32, vp]
    lib.td_logit_edits_ban.argtypes = [vp, i32, vp, i32, i32, vp]
    lib.td_logit_edits_allow_only.argtypes = [vp, i32, vp, i32, vp]
    lib.td_logit_edits_read.argtypes = [vp, i32, vp, vp, vp]
    lib.td_sample_rows_edit_bf16.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp, i32, vp, vp]
    lib.td_logprobs_rows_bf16.argtypes = [vp, i64, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    return lib


def test_abi_version_and_the_pinned_struct():
    lib = _lib()
    assert lib.td_abi_version() > 14
    assert lib.td_sample_row_size() == 48


def test_edit_state_argument_errors_come_before_any_hip_call():
    lib = _lib()
    h = ctypes.c_void_p()
    for n_slots, vocab, word in ((0, 4096, "n_slots"), (70000, 4096, "n_slots"), (4, 4100, "vocab"), (4, 0, "vocab")):
        assert lib.td_logit_edits_create(n_slots, vocab, ctypes.byref(h)) == TD_ERR_INVALID and word in lib.td_last_error().decode()
        assert not h.value
    assert lib.td_logit_edits_create(4, 4096, None) == TD_ERR_INVALID
    one = ctypes.c_void_p(256)
    assert lib.td_logit_edits_reset_slot(None, 0, None) == TD_ERR_INVALID and "null edit state" in lib.td_last_error().decode()
    assert lib.td_logit_edits_set_bias(None, 0, one, one, 1, None) == TD_ERR_INVALID
    assert lib.td_logit_edits_ban(None, 0, one, 1, 1, None) == TD_ERR_INVALID
    assert lib.td_logit_edits_allow_only(None, 0, one, 1, None) == TD_ERR_INVALID
    assert lib.td_logit_edits_read(None, 0, one, one, None) == TD_ERR_INVALID
    lib.td_logit_edits_destroy.argtypes = [ctypes.c_void_p]
    lib.td_logit_edits_destroy.restype = None
    lib.td_logit_edits_destroy(None)                         # a null handle is a no-op


def test_sample_rows_edit_with_a_null_state_is_sample_rows_and_checks_like_it():
    lib = _lib()
    one = ctypes.c_void_p(256)                           # never dereferenced
    ok = dict(logits=one, ld=4096, rows=4, vocab=4096, params=one, offsets=one, update=0, out=one)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.td_sample_rows_edit_bf16(None, None, None, a["logits"], a["ld"], a["rows"], a["vocab"], a["params"], a["offsets"], a["update"], a["out"], None)
        return rc, lib.td_last_error().decode()

    for name in ("logits", "params", "offsets", "out"):
        rc, msg = call(**{name: None})
        assert rc == TD_ERR_INVALID and "null pointer" in msg, name
    for kw in (dict(vocab=4100), dict(ld=4100), dict(logits=ctypes.c_void_p(264))):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "multiples of 8" in msg, kw
    rc, msg = call(rows=0)
    assert rc == TD_ERR_INVALID and "1..65535 rows" in msg
    rc, msg = call(update=1)
    assert rc == TD_ERR_INVALID and "update_state" in msg


def test_logprobs_argument_errors_come_before_any_hip_call():
    lib = _lib()
    one = ctypes.c_void_p(256)
    ok = dict(logits=one, ld=4096, rows=4, vocab=4096, ids=one, n_top=one, cap=20, lp=one, rank=one, tid=one, tlp=one)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.td_logprobs_rows_bf16(a["logits"], a["ld"], a["rows"], a["vocab"], a["ids"], a["n_top"], a["cap"], a["lp"], a["rank"], a["tid"], a["tlp"], None)
        return rc, lib.td_last_error().decode()

    for name in ("logits", "ids", "n_top", "lp", "rank"):
        rc, msg = call(**{name: None})
        assert rc == TD_ERR_INVALID and "null pointer" in msg, name
    for cap in (-1, 21):
        rc, msg = call(cap=cap)
        assert rc == TD_ERR_INVALID and "top_cap" in msg
    rc, msg = call(tid=None)
    assert rc == TD_ERR_INVALID and "top_ids" in msg
    for kw in (dict(vocab=4100), dict(ld=4100), dict(ld=4088), dict(logits=ctypes.c_void_p(264))):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "multiples of 8" in msg, kw
    for rows in (0, 65536):
        rc, msg = call(rows=rows)
        assert rc == TD_ERR_INVALID and "1..65535 rows" in msg


def test_op_schemas():
    import thinkdiff.ops as ops
    ops.register()
    assert str(torch.ops.thinkdiff_hip.sample_rows_edit.default._schema) == \
        "thinkdiff_hip::sample_rows_edit(Tensor logits, Tensor params, Tensor offsets, int? state, bool update_state, int? edits, Tensor? edit_slots) -> Tensor"
    assert str(torch.ops.thinkdiff_hip.logprobs_rows.default._schema) == \
        "thinkdiff_hip::logprobs_rows(Tensor logits, Tensor ids, Tensor n_top, int top_cap) -> (Tensor, Tensor, Tensor, Tensor)"
    assert str(torch.ops.thinkdiff_hip.sample_rows.default._schema) == \
        "thinkdiff_hip::sample_rows(Tensor logits, Tensor params, Tensor offsets, int? state, bool update_state) -> Tensor", "the existing schema does not change"
    for name in ("sample_rows_edit", "logprobs_rows"):
        assert str(getattr(torch.ops.thinkdiff_hip, name).default._schema) == f"thinkdiff_hip::{name}{ops.SCHEMAS[name]}"
    with pytest.raises((NotImplementedError, RuntimeError)):      # no host kernel to fall back to
        torch.ops.thinkdiff_hip.logprobs_rows(torch.zeros(1, 8, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 5)


# ---- the ban planner against brute force --------------------------------------------------------------------------------------
V = 40


class _Slot:
    """What the device slot would hold: applies the planner's calls the way td_logit_edits_* do."""

    def __init__(self, plan):
        allowed, ban = plan.start()
        self.banned = set(range(V)) - set(allowed) if allowed is not None else set()
        self.banned |= set(ban)

    def apply(self, on, off):
        assert not (set(on) & set(off))
        self.banned -= set(off)
        self.banned |= set(on)


@pytest.mark.parametrize("seed", range(12))
def test_ban_planner_matches_brute_force_on_random_streams(seed):
    from thinkdiff.models.qwen2_vl import LogitEditPlan, SamplingParams
    rng = random.Random(seed)
    # overlapping words over a small alphabet (so prefixes match often), one-token words, words that share their last token, a word inside a word
    alphabet = list(range(6))
    words = [[rng.choice(alphabet) for _ in range(rng.randint(1, 4))] for _ in range(rng.randint(2, 7))] + [[1, 2], [2, 1, 2], [0, 0, 0, 0], [3, 2]]
    one_token = {w[0] for w in words if len(w) == 1}
    stop_ids = [rng.choice(alphabet), 17] + ([next(iter(one_token))] if one_token and seed % 2 else [])      # a stop id that is also a bad word ...
    allowed = None
    if seed % 3 == 0:
        allowed = sorted(set(alphabet) - {stop_ids[0]} | {20, 21})                                              # ... or lies outside the allowed set
    eos, ignore_eos, min_tokens = 5, bool(seed % 4 == 0), rng.randint(0, 9)
    sp = SamplingParams(allowed_token_ids=allowed, bad_words_token_ids=words, stop_token_ids=stop_ids, min_tokens=min_tokens, max_tokens=64,
                        ignore_eos=ignore_eos, mask_stop_below_min_tokens=True).validate()
    plan = LogitEditPlan(sp, V, eos)
    assert plan.needs_tokens == any(len(w) > 1 for w in words)
    slot = _Slot(plan)
    kw = dict(allowed=allowed, bad_words=words, stop_ids=stop_ids, min_tokens=min_tokens, eos=eos, ignore_eos=ignore_eos)
    output = []
    assert slot.banned == E.banned_at(output, V, **kw)
    for _ in range(60):
        output.append(rng.choice(alphabet))
        before = set(slot.banned)
        on, off = plan.advance(output[-1])
        slot.apply(on, off)
        want = E.banned_at(output, V, **kw)
        assert slot.banned == want, (output, sorted(slot.banned ^ want))
        assert set(on) == want - before and set(off) == before - want, "only the differences are sent"


def test_ban_planner_never_unbans_what_another_rule_holds():
    from thinkdiff.models.qwen2_vl import LogitEditPlan, SamplingParams
    # token 7: a stop id (masked for 2 tokens), a one-token bad word and the last token of [3, 7]; token 9: a stop id outside the allowed set
    sp = SamplingParams(allowed_token_ids=[3, 4, 7, 8], bad_words_token_ids=[[7], [3, 7], [3, 8]], stop_token_ids=[7, 9, 4], min_tokens=2,
                        mask_stop_below_min_tokens=True).validate()
    plan = LogitEditPlan(sp, V, None)
    allowed, ban = plan.start()
    assert allowed == [3, 4, 7, 8] and ban == [4, 7]
    assert plan.advance(3) == ([8], [])              # [3, 8] matched; 7 is already banned for good
    assert plan.advance(4) == ([], [4, 8])           # min_tokens reached: 4 is released, 7 and 9 are not (a bad word; outside the allowed set)
    assert plan.advance(3) == ([8], [])
    assert plan.advance(3) == ([], [])
    assert plan.advance(8) == ([], [8])
    # min-tokens alone: no token needed on the host
    plan = LogitEditPlan(SamplingParams(stop_token_ids=[5], min_tokens=3, mask_stop_below_min_tokens=True, ignore_eos=False), V, 6)
    assert not plan.needs_tokens and plan.per_step and plan.start() == (None, [5, 6])
    assert [plan.advance() for _ in range(4)] == [([], []), ([], []), ([], [5, 6]), ([], [])]


def test_ban_planner_admission_errors():
    from thinkdiff.models.qwen2_vl import LogitEditPlan, SamplingParams
    for kw, field in ((dict(logit_bias={V: 1.0}), "logit_bias"), (dict(allowed_token_ids=[1, V + 3]), "allowed_token_ids"),
                      (dict(bad_words_token_ids=[[1, V]]), "bad_words_token_ids")):
        with pytest.raises(ValueError, match=f"SamplingParams.{field}.*outside the vocabulary of {V}"):
            LogitEditPlan(SamplingParams(**kw).validate(), V, None)
    with pytest.raises(ValueError, match="allowed_token_ids.*nothing could be sampled"):
        LogitEditPlan(SamplingParams(allowed_token_ids=[1, 2], bad_words_token_ids=[[1], [2]]).validate(), V, None)
    with pytest.raises(ValueError, match="allowed_token_ids.*nothing could be sampled"):
        LogitEditPlan(SamplingParams(allowed_token_ids=[1, 2], bad_words_token_ids=[[1]], stop_token_ids=[2], min_tokens=4, mask_stop_below_min_tokens=True).validate(), V, None)


# ---- routing: a stand-in engine ----------------------------------------------------------------------------------------------------
class _Edits:
    """Stands in for thinkdiff._hip.LogitEdits: keeps each slot's banned set and bias and records the calls."""
    handle = 0xED17

    def __init__(self, vocab):
        self.vocab, self.banned, self.bias, self.calls = vocab, {}, {}, []

    def reset_slot(self, slot):
        self.calls.append(("reset", slot))
        self.banned[slot], self.bias[slot] = set(), {}

    def set_bias(self, slot, bias):
        self.calls.append(("bias", slot))
        self.bias[slot] = dict(bias)

    def ban(self, slot, ids, on=True):
        self.calls.append(("ban", slot, list(ids), bool(on)))
        self.banned[slot] = (self.banned[slot] | set(ids)) if on else (self.banned[slot] - set(ids))

    def allow_only(self, slot, ids):
        self.calls.append(("allow", slot))
        self.banned[slot] = set(range(self.vocab)) - set(ids)


def _fake_engine(n_slots, vocab=97, D=8):
    """A toy model whose logits prefer (7 t + 3) mod vocab after token t, then (7 t + 4), ...: greedy under edits is computable by hand."""
    from thinkdiff.models import qwen2_vl as Q
    calls = SimpleNamespace(top_p=0, rows=0, edit=0, logprobs=0)

    class Fake(Q.Qwen2VLTextEngine):
        def __init__(self):
            self.config = SimpleNamespace(hidden_size=D, vocab_size=vocab)
            self.device = torch.device("cpu")
            self.n_slots, self.slot_len, self.prefill_rows = n_slots, 64, 96
            self.edits = _Edits(vocab)

        def __del__(self):
            pass

        def _logit_edits(self):
            return self.edits

        def embed_tokens(self, token_ids):
            out = torch.zeros(len(token_ids), D, dtype=torch.bfloat16)
            out[:, 0] = torch.tensor(list(token_ids), dtype=torch.float32)
            return out

        @staticmethod
        def _logits_for(tok, row):
            first = (int(tok) * 7 + 3) % vocab
            row.copy_((8.0 - ((torch.arange(vocab) - first) % vocab).float() * 0.0625).bfloat16())

        def forward(self, position_ids, token_ids=None, inputs_embeds=None, pos0=0, want_hidden=True, want_logits=False, slot=0):
            lg = torch.empty(vocab, dtype=torch.bfloat16)
            self._logits_for(int(token_ids[-1]), lg)
            return self.embed_tokens(token_ids.tolist()), lg

        def decode_batch(self, token_ids, position_ids, cache_pos, want_logits=True, slots=None):
            tok = torch.as_tensor(token_ids, dtype=torch.int32)
            hid, lg = torch.zeros(len(tok), D, dtype=torch.bfloat16), torch.empty(len(tok), vocab, dtype=torch.bfloat16)
            for i, t in enumerate(tok.tolist()):
                self._logits_for(t, lg[i])
            return hid, lg

        def _prefill_packed_slots(self, k, slots_c, emb, pos, lens_c, hid_out, logits_out):
            r = 0
            for b, n in enumerate(list(lens_c)):
                hid_out[r:r + n] = emb[r:r + n]
                self._logits_for(int(emb[r + n - 1, 0]), logits_out[b])
                r += n

        def _decode_slots(self, n, slots_np, tok_dev, pos_dev, cache_np, hid_out, logits_out):
            for i in range(n):
                hid_out[i].zero_()
                hid_out[i, 0] = float(tok_dev[i])
                self._logits_for(int(tok_dev[i]), logits_out[i])

    e = Fake()

    def sample_top_p(logits, temperature, top_p, key, step):
        calls.top_p += 1
        return logits.float().argmax(dim=1).to(torch.int32)

    def sample_rows(logits, params, offsets, state, update_state):
        calls.rows += 1
        return logits.float().argmax(dim=1).to(torch.int32)

    def sample_rows_edit(logits, params, offsets, state, update_state, edits, edit_slots):
        calls.edit += 1
        assert edits == _Edits.handle and edit_slots.dtype == torch.int32 and edit_slots.numel() == logits.shape[0]
        z = logits.float().clone()
        for i, s in enumerate(edit_slots.tolist()):
            if s >= 0:
                for t, b in e.edits.bias[s].items():
                    z[i, t] += b
                if e.edits.banned[s]:
                    z[i, sorted(e.edits.banned[s])] = float("-inf")
        return z.argmax(dim=1).to(torch.int32)

    def logprobs_rows(logits, ids, n_top, top_cap):
        calls.logprobs += 1
        lp = torch.log_softmax(logits.float(), dim=-1)
        n = logits.shape[0]
        top = torch.sort(logits.float(), dim=-1, descending=True, stable=True).indices[:, :top_cap].to(torch.int32)
        chosen = lp[torch.arange(n), ids.long()]
        rank = (logits.float() >= logits.float()[torch.arange(n), ids.long()][:, None]).sum(-1).to(torch.int32)
        return chosen, rank, top, torch.gather(lp, 1, top.long())

    ops = SimpleNamespace(sample_top_p=sample_top_p, sample_rows=sample_rows, sample_rows_edit=sample_rows_edit, logprobs_rows=logprobs_rows)
    return e, Q, ops, calls


def _patch(monkeypatch, Q, ops):
    monkeypatch.setattr(Q, "_OPS", ops)
    monkeypatch.setattr(Q.Qwen2VLTextEngine, "_draw_sampler_key", staticmethod(lambda generator=None: 1))


def _greedy(prompt, n, vocab=97, banned_fn=lambda out: set(), bias=None):
    out, t = [], prompt[-1]
    for _ in range(n):
        first = (t * 7 + 3) % vocab
        z = {u: 8.0 - ((u - first) % vocab) * 0.0625 + (bias or {}).get(u, 0.0) for u in range(vocab)}
        ban = banned_fn(out)
        t = max((u for u in range(vocab) if u not in ban), key=lambda u: (z[u], -u))
        out.append(t)
    return out


def test_requests_with_edits_route_through_sample_rows_edit_and_the_others_do_not(monkeypatch):
    from thinkdiff.models.qwen2_vl import SamplingParams
    e, Q, ops, calls = _fake_engine(4)
    _patch(monkeypatch, Q, ops)
    prompts = [[1, 2, 3], [10, 11], [20], [30, 31, 32, 33], [40, 41]]
    plain = [_greedy(p, 8) for p in prompts]
    w2 = plain[1][2:4]                                        # a two-token bad word out of request 1's plain continuation
    sps = [SamplingParams(temperature=0.0, max_tokens=8, min_tokens=8, bad_words_token_ids=[[plain[0][0]]]),
           SamplingParams(temperature=0.0, max_tokens=8, min_tokens=8, bad_words_token_ids=[w2]),
           SamplingParams(temperature=0.0, max_tokens=8, min_tokens=8),
           SamplingParams(temperature=0.0, max_tokens=8, min_tokens=6, stop_token_ids=[plain[3][1]], mask_stop_below_min_tokens=True, logit_bias={5: 100.0}),
           SamplingParams(temperature=0.0, max_tokens=8, min_tokens=8, allowed_token_ids=list(range(0, 97, 6)), logprobs=2)]
    reqs = [{"prompt_token_ids": p} for p in prompts]
    out = e.generate_continuous(reqs, sps, max_live=2)        # five requests over two slots: every slot is reused
    assert calls.top_p == 0 and calls.edit > 0
    got = [o["token_ids"] for o in out]
    assert got[0] == _greedy(prompts[0], 8, banned_fn=lambda o: {plain[0][0]}) and plain[0][0] not in got[0]
    assert got[1] == _greedy(prompts[1], 8, banned_fn=lambda o: {w2[1]} if o[-1:] == w2[:1] else set())
    assert got[1][:3] == plain[1][:3] and got[1][3] != plain[1][3]
    assert got[2] == plain[2], "a request without edits in a reused slot samples plainly"
    assert got[3] == _greedy(prompts[3], 8, banned_fn=lambda o: {plain[3][1]} if len(o) < 6 else set(), bias={5: 100.0})
    assert plain[3][1] not in got[3][:6] and got[3][0] == 5
    assert all(t % 6 == 0 for t in got[4]) and len(got[4]) == 8
    assert "logprobs" not in out[0] and "cumulative_logprob" not in out[3]
    assert len(out[4]["logprobs"]) == 8 and all(len(d) in (2, 3) for d in out[4]["logprobs"])
    assert out[4]["cumulative_logprob"] == pytest.approx(sum(d[t].logprob for d, t in zip(out[4]["logprobs"], got[4])))
    # every admission of an edited request reset its slot first
    resets = [c for c in e.edits.calls if c[0] == "reset"]
    assert len(resets) == 4
    # the same requests one by one and as a batch
    for i in (0, 1, 3, 4):
        assert e.generate(prompts[i], sps[i])["token_ids"] == got[i]
    e2, Q2, ops2, calls2 = _fake_engine(8)
    _patch(monkeypatch, Q2, ops2)
    e2.packed_prefill, e2.prefill_rows = False, 4             # (the stand-in has no batched prefill: one forward per request)
    assert [o["token_ids"] for o in e2.generate_batch(reqs, sps)] == got


def test_no_live_edit_means_the_old_calls(monkeypatch):
    from thinkdiff.models.qwen2_vl import SamplingParams
    e, Q, ops, calls = _fake_engine(4)
    _patch(monkeypatch, Q, ops)
    reqs = [{"prompt_token_ids": [i + 1, i + 2]} for i in range(3)]
    e.generate_continuous(reqs, [SamplingParams(temperature=0.0, max_tokens=3, min_tokens=3, top_k=4)] * 3, max_live=4)
    assert calls.rows > 0 and calls.edit == calls.top_p == calls.logprobs == 0 and e.edits.calls == []
    out = e.generate_continuous(reqs, SamplingParams(temperature=0.0, max_tokens=3, min_tokens=3, logprobs=0), max_live=4)
    assert calls.top_p > 0 and calls.edit == 0 and calls.logprobs == 3, "logprobs alone: the old sampler plus one logprobs launch per step"
    assert all(len(o["logprobs"]) == 3 and all(len(d) == 1 for d in o["logprobs"]) for o in out)
    # forced tokens are scored
    forced = [[5, 6, 7], [8, 9], [10]]
    out = e.generate_continuous(reqs, SamplingParams(max_tokens=3, min_tokens=3, logprobs=1), forced_output_ids=forced, max_live=4)
    assert [o["token_ids"] for o in out] == forced and [len(o["logprobs"]) for o in out] == [3, 2, 1]
    assert all(t in d for o, f in zip(out, forced) for d, t in zip(o["logprobs"], f))
    with pytest.raises(ValueError, match="outside the vocabulary of 97"):
        e.generate(reqs[0]["prompt_token_ids"], SamplingParams(logit_bias={97: 1.0}))


# ---- vllm_config ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_path", ["thinkdiff.models.mllama_vllm_t5_embed_decoder_2:MllamaVllmT5EmbedDecoderForConditionalGeneration_5",
                                      "thinkdiff.models.mllama_vllm_generate_1:MllamaVllmGenerate_1"])
def test_vllm_config_edit_keys_reach_sampling_params_and_refused_keys_raise(cls_path, monkeypatch):
    mod_name, name = cls_path.split(":")
    mod = importlib.import_module(mod_name)

    class Engine(mod.Qwen2VLTextEngine):      # no HIP handle
        def __init__(self, *a, **kw):
            pass

        def __del__(self):
            pass

    monkeypatch.setattr(mod, "Qwen2VLTextEngine", Engine)
    if hasattr(mod, "HipVisionProjector"):
        monkeypatch.setattr(mod, "HipVisionProjector", lambda *a, **kw: None)
    cls = getattr(mod, name)
    base = cls(vllm_config={"max_model_len": 64}).mllama_sampling_params
    assert not base.has_edit and base.logprobs is None
    sp = cls(vllm_config={"max_model_len": 64, "logit_bias": {7: -3.5}, "allowed_token_ids": [7, 8, 9], "bad_words_token_ids": [[8], [7, 9]],
                          "mask_stop_below_min_tokens": True, "logprobs": 5}).mllama_sampling_params
    assert (sp.logit_bias, sp.allowed_token_ids, sp.bad_words_token_ids, sp.mask_stop_below_min_tokens, sp.logprobs) == ({7: -3.5}, [7, 8, 9], [[8], [7, 9]], True, 5)
    assert sp.has_edit and sp.per_request
    with pytest.raises(ValueError, match="prompt_logprobs"):
        cls(vllm_config={"max_model_len": 64, "prompt_logprobs": 1})
    with pytest.raises(ValueError, match="bad_words_token_ids"):
        cls(vllm_config={"max_model_len": 64, "bad_words": ["foo"]})
    with pytest.raises(ValueError, match=r"SamplingParams.logprobs=50"):
        cls(vllm_config={"max_model_len": 64, "logprobs": 50})
