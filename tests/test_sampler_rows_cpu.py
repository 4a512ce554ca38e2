"""The per-request sampler without a GPU: SamplingParams.validate, the one-SamplingParams-per-request form of the three generate entries, the routing
between td_sample_top_p_bf16 and td_sample_rows_bf16 (a stand-in engine in the pattern of tests/test_scheduler_cpu.py, which also checks the row
table and the history resets the scheduler hands to the sampler on every step), the vllm_config pass-through of the two model classes, the argument
errors of the C ABI, and the restatement of the rule (tests/sampler_rows_common.py) on rows small enough to do by hand."""
import ctypes
import importlib
import os
from types import SimpleNamespace

import pytest
import torch

import sampler_rows_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
TD_ERR_INVALID = 2
V, D = 97, 8
KEY = 1      # what the stubbed _draw_sampler_key returns


def _next(tok):      # the toy model's greedy continuation
    return (int(tok) * 7 + 3) % V


# ---- SamplingParams ----------------------------------------------------------------------------------------------------
def test_defaults_are_vllms_and_route_to_the_old_sampler():
    from thinkdiff.models.qwen2_vl import SamplingParams
    sp = SamplingParams()
    assert (sp.top_k, sp.min_p, sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.seed) == (-1, 0.0, 1.0, 0.0, 0.0, None)
    assert sp.validate() is sp and not sp.per_request and not sp.has_penalty
    assert not SamplingParams(top_k=0).per_request            # vLLM: 0 and -1 both mean "off"
    for kw in (dict(top_k=5), dict(min_p=0.1), dict(repetition_penalty=1.1), dict(presence_penalty=0.5), dict(frequency_penalty=-0.5), dict(seed=0)):
        assert SamplingParams(**kw).validate().per_request, kw
    assert SamplingParams(seed=3).has_penalty is False and SamplingParams(frequency_penalty=0.1).has_penalty


@pytest.mark.parametrize("field,value", [("top_k", -2), ("top_k", 1.5), ("min_p", -0.1), ("min_p", 1.5), ("top_p", 0.0), ("top_p", 1.01),
                                         ("repetition_penalty", 0.0), ("repetition_penalty", -1.0), ("presence_penalty", 2.5),
                                         ("presence_penalty", -2.01), ("frequency_penalty", 3.0), ("frequency_penalty", float("nan")),
                                         ("temperature", -0.5), ("seed", 1.5), ("min_p", float("inf"))])
def test_validate_names_the_field_and_value(field, value):
    from thinkdiff.models.qwen2_vl import SamplingParams
    with pytest.raises(ValueError) as e:
        SamplingParams(**{field: value}).validate()
    assert f"SamplingParams.{field}=" in str(e.value) and repr(value) in str(e.value)


# ---- the restatement, by hand --------------------------------------------------------------------------------------------
def test_restatement_top_p_works_on_the_top_k_mass():
    p = torch.tensor([0.40, 0.25, 0.15, 0.10, 0.06, 0.04], dtype=torch.float64)
    z = p.log()
    # top-3 mass 0.80; top_p 0.7 of it = 0.56: mass in front of token 1 is 0.40 < 0.56 (kept), in front of token 2 is 0.65 (dropped)
    q, edge, _ = C.law(z, 1.0, top_k=3, top_p=0.7)
    assert (q > 0).tolist() == [True, True, False, False, False, False]
    assert torch.allclose(q[:2], torch.tensor([0.40, 0.25], dtype=torch.float64) / 0.65) and abs(edge - 0.25) < 1e-12
    # top-p of the WHOLE mass would have kept token 2 as well (0.65 < 0.70): the order matters
    q_all, _, _ = C.law(z, 1.0, top_k=-1, top_p=0.7)
    assert int((q_all > 0).sum()) == 3
    q_k, _, _ = C.law(z, 1.0, top_k=3)
    assert torch.allclose(q_k[:3], p[:3] / 0.80) and float(q_k[3:].sum()) == 0.0
    assert int((C.law(z, 1.0, top_k=0)[0] > 0).sum()) == 6 and int((C.law(z, 1.0, top_k=6)[0] > 0).sum()) == 6      # off


def test_restatement_repetition_penalty_sign_rule_and_order():
    x = torch.tensor([2.0, -2.0, 1.0, -1.0, 3.0, 0.5, -0.5, 4.0]).bfloat16()
    counts = torch.tensor([0, 0, 3, 1, 0, 0, 0, 0])
    z = C.penalise(x, prompt_ids=[0, 1, 200, -4], counts=counts, repetition_penalty=2.0, presence_penalty=0.25, frequency_penalty=0.5)
    # prompt-only tokens 0, 1: repetition only (positive divided, negative multiplied); generated tokens 2, 3: all three; others untouched
    assert z.tolist() == [1.0, -4.0, 0.5 - 1.5 - 0.25, -2.0 - 0.5 - 0.25, 3.0, 0.5, -0.5, 4.0]
    assert z.dtype == torch.float32
    # greedy after the penalties: a penalised former maximum is not the maximum
    z2 = C.penalise(x, prompt_ids=[7], repetition_penalty=2.0)
    assert int(x.float().argmax()) == 7 and int(z2.argmax()) == 4 and float(z2[7]) == 2.0


def test_restatement_pins_min_p_after_top_p():
    p = torch.tensor([0.30, 0.28, 0.20, 0.10, 0.05, 0.04, 0.02, 0.01], dtype=torch.float64)
    z = p.log()
    # min-p 0.3 keeps p >= 0.09: {0, 1, 2, 3}, mass 0.88.  The masses in front of tokens 0.. are 0, 0.30, 0.58, 0.78, 0.88, 0.93, ..
    # engine order, top_p 0.7: {0, 1, 2} (0.58 < 0.70 <= 0.78), and min-p agrees
    q, _, _ = C.law(z, 1.0, top_p=0.7, min_p=0.3)
    assert (q > 0).tolist() == [True, True, True] + [False] * 5
    # top_p 0.9: top-p keeps {0..4} (0.88 < 0.90), min-p then drops token 4 (0.05 < 0.09); min-p first gives 0.9 x 0.88 = 0.792 > 0.78: the same set
    q_eng, _, _ = C.law(z, 1.0, top_p=0.9, min_p=0.3)
    q_new, _, _ = C.law(z, 1.0, top_p=0.9, min_p=0.3, min_p_first=True)
    assert (q_eng > 0).tolist() == (q_new > 0).tolist() == [True] * 4 + [False] * 4
    # top_p 0.62 is where the two orders part: of the whole mass it keeps token 2 (0.58 < 0.62); of the min-p survivors it is 0.5456 <= 0.58 and
    # token 2 is dropped.  The engine implements the first.
    q_eng, _, _ = C.law(z, 1.0, top_p=0.62, min_p=0.3)
    q_new, _, _ = C.law(z, 1.0, top_p=0.62, min_p=0.3, min_p_first=True)
    assert int((q_eng > 0).sum()) == 3 and int((q_new > 0).sum()) == 2


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def _lib():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    lib.td_sample_row_size.restype = ctypes.c_size_t
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.td_sample_rows_bf16.argtypes = [vp, vp, i64, i32, i32, vp, vp, i32, vp, vp]
    lib.td_sampler_create.argtypes = [i32, i32, vp]
    return lib


def test_struct_size_matches_the_binding():
    from thinkdiff import _hip
    assert _lib().td_sample_row_size() == ctypes.sizeof(_hip.TdSampleRow) == 48
    t = _hip.pack_sample_rows([dict(top_k=7, seed=2 ** 64 - 3, slot=5, stream=9, min_p=0.25), {}])
    assert t.shape == (2, 48) and t.dtype == torch.uint8
    back = (_hip.TdSampleRow * 2).from_buffer_copy(t.numpy().tobytes())
    assert (back[0].top_k, back[0].seed, back[0].slot, back[0].stream, back[0].min_p) == (7, 2 ** 64 - 3, 5, 9, 0.25)
    assert (back[1].top_k, back[1].slot, back[1].top_p, back[1].repetition_penalty) == (-1, -1, 1.0, 1.0)
    with pytest.raises(_hip.ThinkDiffHipError, match="topk"):
        _hip.pack_sample_rows([dict(topk=3)])


def test_sample_rows_argument_errors_come_before_any_hip_call():
    lib = _lib()
    one = ctypes.c_void_p(256)                           # never dereferenced
    ok = dict(s=None, logits=one, ld=4096, rows=4, vocab=4096, params=one, offsets=one, update=0, out=one)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.td_sample_rows_bf16(a["s"], a["logits"], a["ld"], a["rows"], a["vocab"], a["params"], a["offsets"], a["update"], a["out"], None)
        return rc, lib.td_last_error().decode()

    for name in ("logits", "params", "offsets", "out"):
        rc, msg = call(**{name: None})
        assert rc == TD_ERR_INVALID and "null pointer" in msg, name
    for kw in (dict(vocab=4100), dict(ld=4100), dict(logits=ctypes.c_void_p(264))):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "multiples of 8" in msg and "16-byte" in msg, kw
    for rows in (0, -1, 65536):
        rc, msg = call(rows=rows)
        assert rc == TD_ERR_INVALID and "1..65535 rows" in msg
    rc, msg = call(update=1)
    assert rc == TD_ERR_INVALID and "update_state" in msg


def test_sampler_state_argument_errors_come_before_any_hip_call():
    lib = _lib()
    h = ctypes.c_void_p()
    for n_slots, vocab, word in ((0, 4096, "n_slots"), (70000, 4096, "n_slots"), (4, 4100, "vocab"), (4, 0, "vocab")):
        assert lib.td_sampler_create(n_slots, vocab, ctypes.byref(h)) == TD_ERR_INVALID and word in lib.td_last_error().decode()
        assert not h.value
    assert lib.td_sampler_create(4, 4096, None) == TD_ERR_INVALID
    one = ctypes.c_void_p(256)
    assert lib.td_sampler_reset_slot(None, 0, None, 0, None) == TD_ERR_INVALID and "null sampler" in lib.td_last_error().decode()
    assert lib.td_sampler_read_counts(None, 0, one, None) == TD_ERR_INVALID
    assert lib.td_sampler_read_prompt_mask(None, 0, one, None) == TD_ERR_INVALID
    assert lib.td_sampler_set_counts(None, 0, one, None) == TD_ERR_INVALID
    lib.td_sampler_destroy.argtypes = [ctypes.c_void_p]
    lib.td_sampler_destroy.restype = None
    lib.td_sampler_destroy(None)                         # a null handle is a no-op


def test_op_schema_takes_an_optional_state_handle():
    import thinkdiff.ops as ops
    ops.register()
    s = str(torch.ops.thinkdiff_hip.sample_rows.default._schema)
    assert "int? state" in s and "bool update_state" in s and "Tensor params" in s and "Tensor offsets" in s
    with pytest.raises((NotImplementedError, RuntimeError)):      # no host kernel to fall back to
        torch.ops.thinkdiff_hip.sample_rows(torch.zeros(1, 8, dtype=torch.bfloat16), torch.zeros(1, 48, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), None, False)


# ---- routing: a stand-in engine that checks what the scheduler hands to the sampler ----------------------------------------------
class _History:
    """Stands in for thinkdiff._hip.Sampler: records the resets."""
    handle = 0xBEEF

    def __init__(self):
        self.resets = []

    def reset_slot(self, slot, prompt_ids=None):
        self.resets.append((int(slot), [int(t) for t in (prompt_ids or [])]))


def _fake_engine(n_slots, requests, sps, slot_len=64, prefill_rows=96):
    """requests have distinct prompts, so a cache slot identifies its request.  sps: the SamplingParams of request i (for the checks only)."""
    from thinkdiff import _hip
    from thinkdiff.models import qwen2_vl as Q
    by_prompt = {tuple(r["prompt_token_ids"]): i for i, r in enumerate(requests)}
    assert len(by_prompt) == len(requests)
    calls = SimpleNamespace(top_p=0, rows=0, pending=None, steps=0, first_sample={})

    class Fake(Q.Qwen2VLTextEngine):
        def __init__(self):      # no HIP handle: only what the scheduler touches
            self.config = SimpleNamespace(hidden_size=D, vocab_size=V)
            self.device = torch.device("cpu")
            self.n_slots, self.slot_len, self.prefill_rows = n_slots, slot_len, prefill_rows
            self.cache, self.slot_req, self.history = {}, {}, _History()

        def __del__(self):
            pass

        def _sampler_state(self):
            return self.history

        def embed_tokens(self, token_ids):
            out = torch.zeros(len(token_ids), D, dtype=torch.bfloat16)
            out[:, 0] = torch.tensor(list(token_ids), dtype=torch.float32)
            return out

        def _logits_for(self, tok, row):
            row.zero_()
            row[_next(tok)] = 8.0

        def _prefill_packed_slots(self, k, slots_c, emb, pos, lens_c, hid_out, logits_out):
            r = 0
            for b, (s, n) in enumerate(zip(list(slots_c), list(lens_c))):
                toks = [int(t) for t in emb[r:r + n, 0].float().tolist()]
                self.cache[s], self.slot_req[s] = toks, by_prompt[tuple(toks)]
                hid_out[r:r + n] = emb[r:r + n]
                self._logits_for(toks[-1], logits_out[b])
                r += n

        def _decode_slots(self, n, slots_np, tok_dev, pos_dev, cache_np, hid_out, logits_out):
            slots = [int(x) for x in slots_np[:n]]
            assert len(set(slots)) == n
            if calls.pending is not None:      # the table of the sample_rows call that produced tok_dev: row i belongs to the sequence in slots[i]
                table, offsets, state, update = calls.pending
                calls.pending = None
                assert len(table) == n == len(offsets)
                any_hist = False
                for i, s in enumerate(slots):
                    req = self.slot_req[s]
                    sp, row = sps[req], table[i]
                    ngen = len(self.cache[s]) - len(requests[req]["prompt_token_ids"])
                    assert (row.top_k, row.min_p, row.temperature) == (sp.top_k, pytest.approx(sp.min_p), pytest.approx(sp.temperature))
                    assert row.repetition_penalty == pytest.approx(sp.repetition_penalty) and row.presence_penalty == pytest.approx(sp.presence_penalty)
                    if sp.seed is not None:
                        assert (row.seed, row.stream, offsets[i]) == (sp.seed, 0, ngen), "a seeded request draws from (its seed, its own token count, 0)"
                    else:
                        assert (row.seed, row.stream, offsets[i]) == (KEY, i, calls.steps), "an unseeded request draws from (key, step, live row)"
                    assert row.slot == (s if sp.has_penalty else -1)
                    any_hist |= sp.has_penalty
                    if sp.has_penalty and ngen == 0:      # its history was reset at admission, on this slot, with its prompt, and not since
                        mine = [x for x in self.history.resets if x[0] == s]
                        assert mine and mine[-1] == (s, requests[req]["prompt_token_ids"])
                        calls.first_sample[req] = len(self.history.resets)
                assert (state == _History.handle) == any_hist and bool(update) == any_hist
            calls.steps += 1
            for i, s in enumerate(slots):
                t = int(tok_dev[i])
                self.cache[s].append(t)
                hid_out[i].zero_()
                hid_out[i, 0], hid_out[i, 1] = float(t), float(s)
                self._logits_for(t, logits_out[i])

    def sample_top_p(logits, temperature, top_p, key, step):
        calls.top_p += 1
        return logits.float().argmax(dim=1).to(torch.int32)

    def sample_rows(logits, params, offsets, state, update_state):
        calls.rows += 1
        n = logits.shape[0]
        assert params.dtype == torch.uint8 and params.numel() == n * ctypes.sizeof(_hip.TdSampleRow) and offsets.dtype == torch.int64
        calls.pending = ((_hip.TdSampleRow * n).from_buffer_copy(params.numpy().tobytes()), offsets.tolist(), state, update_state)
        return logits.float().argmax(dim=1).to(torch.int32)

    return Fake(), Q, SimpleNamespace(sample_top_p=sample_top_p, sample_rows=sample_rows), calls


def _requests(N, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [{"prompt_token_ids": [i] + torch.randint(0, V, (1 + (7 * i) % 20,), generator=g).tolist()} for i in range(N)]      # (distinct first token)


def _expected(prompt, sp, eos):
    exp, t = [], prompt[-1]
    while len(exp) < sp.max_tokens:
        t = _next(t)
        exp.append(t)
        if len(exp) >= sp.min_tokens and (t in (sp.stop_token_ids or []) or (not sp.ignore_eos and t == eos)):
            break
    return exp


def _patch(monkeypatch, Q, ops):
    monkeypatch.setattr(Q, "_OPS", ops)
    monkeypatch.setattr(Q.Qwen2VLTextEngine, "_draw_sampler_key", staticmethod(lambda generator=None: KEY))


@pytest.mark.parametrize("max_live", [2, 5, 16])
def test_a_default_single_sampling_params_calls_only_sample_top_p(max_live, monkeypatch):
    reqs = _requests(20)
    from thinkdiff.models.qwen2_vl import SamplingParams
    sp = SamplingParams(temperature=0.0, max_tokens=10, min_tokens=3, ignore_eos=False, stop_token_ids=list(range(0, V, 4)))
    e, Q, ops, calls = _fake_engine(16, reqs, [sp] * 20)
    _patch(monkeypatch, Q, ops)
    out = e.generate_continuous(reqs, sp, eos_token_id=5, max_live=max_live)
    assert calls.rows == 0 and calls.top_p > 0 and e.history.resets == []
    for r, o in zip(reqs, out):
        assert o["token_ids"] == _expected(r["prompt_token_ids"], sp, 5)


@pytest.mark.parametrize("max_live", [2, 5, 16])
def test_per_request_list_routes_through_sample_rows_with_a_live_row_table(max_live, monkeypatch):
    from thinkdiff.models.qwen2_vl import SamplingParams
    N = 30
    reqs = _requests(N)
    sps = []
    for i in range(N):
        kw = dict(temperature=0.0 if i % 3 else 0.7, max_tokens=4 + (5 * i) % 9, min_tokens=1 + i % 3, ignore_eos=bool(i % 2),
                  stop_token_ids=list(range(i % 5, V, 5 + i % 3)))
        if i % 4 == 1:
            kw.update(seed=1000 + i, top_k=3 + i)
        if i % 4 == 2:
            kw.update(repetition_penalty=1.2, presence_penalty=0.5)
        if i % 4 == 3:
            kw.update(min_p=0.1, frequency_penalty=0.25, seed=7)
        sps.append(SamplingParams(**kw))
    e, Q, ops, calls = _fake_engine(16, reqs, sps)
    _patch(monkeypatch, Q, ops)
    out = e.generate_continuous(reqs, sps, eos_token_id=5, max_live=max_live)
    assert calls.top_p == 0 and calls.rows > 0
    for r, sp, o in zip(reqs, sps, out):      # the stop rules are each request's own
        assert o["token_ids"] == _expected(r["prompt_token_ids"], sp, 5)
    # history: reset exactly once per request with a penalty, none for the others
    assert len(e.history.resets) == sum(sp.has_penalty for sp in sps) == len(calls.first_sample)
    assert sorted(p[0] for _, p in e.history.resets) == [i for i in range(N) if sps[i].has_penalty]


def test_single_non_default_field_routes_through_sample_rows_without_history(monkeypatch):
    from thinkdiff.models.qwen2_vl import SamplingParams
    reqs = _requests(6)
    for kw, hist in ((dict(top_k=5), False), (dict(seed=9), False), (dict(min_p=0.2), False), (dict(repetition_penalty=1.1), True)):
        sp = SamplingParams(temperature=0.0, max_tokens=5, min_tokens=5, **kw)
        e, Q, ops, calls = _fake_engine(4, reqs, [sp] * 6)
        _patch(monkeypatch, Q, ops)
        out = e.generate_continuous(reqs, sp, max_live=4)
        assert calls.top_p == 0 and calls.rows > 0 and bool(e.history.resets) == hist, kw
        assert all(len(o["token_ids"]) == 5 for o in out)


def test_forced_decoding_does_not_sample_and_keeps_no_history(monkeypatch):
    from thinkdiff.models.qwen2_vl import SamplingParams
    reqs = _requests(5)
    sp = SamplingParams(max_tokens=6, min_tokens=6, repetition_penalty=1.3, top_k=4)
    e, Q, ops, calls = _fake_engine(4, reqs, [sp] * 5)
    _patch(monkeypatch, Q, ops)
    forced = [[(3 * i + j) % V for j in range(4)] for i in range(5)]
    out = e.generate_continuous(reqs, sp, forced_output_ids=forced, max_live=4)
    assert [o["token_ids"] for o in out] == forced and calls.rows == calls.top_p == 0 and e.history.resets == []


def test_wrong_list_length_is_a_value_error_before_any_work(monkeypatch):
    from thinkdiff.models.qwen2_vl import SamplingParams
    reqs = _requests(3)
    e, Q, ops, calls = _fake_engine(4, reqs, [])
    _patch(monkeypatch, Q, ops)
    two = [SamplingParams(max_tokens=2, min_tokens=2)] * 2
    with pytest.raises(ValueError, match="2 SamplingParams for 3 request"):
        e.generate_continuous(reqs, two, max_live=4)
    with pytest.raises(ValueError, match="2 SamplingParams for 3 request"):
        e.generate_batch(reqs, two)
    with pytest.raises(ValueError, match="2 SamplingParams for 1 request"):
        e.generate(reqs[0]["prompt_token_ids"], two)
    with pytest.raises(ValueError, match="SamplingParams.top_k=-5"):
        e.generate_batch(reqs, [SamplingParams(), SamplingParams(top_k=-5), SamplingParams()])
    with pytest.raises(ValueError, match="SamplingParams.min_p=2"):
        e.generate(reqs[0]["prompt_token_ids"], SamplingParams(min_p=2))
    with pytest.raises(ValueError, match="more than 2 requests"):      # chunks pulled lazily: refused when the chunk that does not fit arrives
        e.generate_continuous(iter([reqs[:2], reqs[2:]]), two, max_live=4)
    assert calls.rows == calls.top_p == 0 and not e.cache


# ---- vllm_config ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_path", ["thinkdiff.models.mllama_vllm_t5_embed_decoder_2:MllamaVllmT5EmbedDecoderForConditionalGeneration_5",
                                      "thinkdiff.models.mllama_vllm_generate_1:MllamaVllmGenerate_1"])
def test_vllm_config_sampler_keys_reach_sampling_params(cls_path, monkeypatch):
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
    assert (base.top_k, base.min_p, base.repetition_penalty, base.presence_penalty, base.frequency_penalty, base.seed) == (-1, 0.0, 1.0, 0.0, 0.0, None)
    assert not base.per_request
    sp = cls(vllm_config={"max_model_len": 64, "top_k": 20, "min_p": 0.05, "repetition_penalty": 1.05, "presence_penalty": 0.5,
                          "frequency_penalty": -0.25, "seed": 1234, "temperature": 0.7}).mllama_sampling_params
    assert (sp.top_k, sp.min_p, sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.seed) == (20, 0.05, 1.05, 0.5, -0.25, 1234)
    assert sp.temperature == 0.7 and sp.per_request and sp.has_penalty
    assert (sp.max_tokens, sp.min_tokens, sp.ignore_eos) == (base.max_tokens, base.min_tokens, base.ignore_eos)
    with pytest.raises(ValueError, match="SamplingParams.repetition_penalty=0"):
        cls(vllm_config={"max_model_len": 64, "repetition_penalty": 0})
