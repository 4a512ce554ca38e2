"""Automatic prefix caching end to end on the GPU: generate_batch and generate_continuous with the feature on against the same engine with it off, on
forced ids.  Tiny engines as in tests/test_spec_decode_gpu.py (2 layers, hidden 1536, scaled weights); bound between two schedules of one model: the
project's _rel < 5e-3.  A false hit -- a request served from rows that are not its prefix -- misses that bound by orders of magnitude.

Measured on MI355X: worst _rel 1.3e-3 over both entries and both cache formats."""
import pytest
import torch

from test_spec_decode_gpu import SHAPES, VOCAB, _rel, _weights

pytestmark = pytest.mark.gpu

GEN = 4


def _engine(caching, slots=16, max_len=192, kv="auto", shape="2b"):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    cfg = Qwen2VLTextConfig(num_hidden_layers=2, intermediate_size=2048, vocab_size=VOCAB, **SHAPES[shape])
    e = Qwen2VLTextEngine(cfg, max_model_len=max_len, n_slots=slots, prefill_rows=1024, kv_cache_dtype=kv, enable_prefix_caching=caching)
    e.load_state_dict(_weights(shape, 7))
    return e


def _family(seed, n=6, shared=96, tails=(5, 12, 19, 26, 33, 40)):
    g = torch.Generator().manual_seed(seed)
    head = torch.randint(0, VOCAB, (shared,), generator=g).tolist()
    return [{"prompt_token_ids": head + [(seed + 31 * i) % VOCAB] + torch.randint(0, VOCAB, (tails[i % len(tails)] - 1,), generator=g).tolist()} for i in range(n)]


def _forced(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (GEN,), generator=g).tolist() for _ in range(n)]


def _run(e, entry, reqs, forced):
    from thinkdiff.models.qwen2_vl import SamplingParams
    sp = SamplingParams(max_tokens=GEN, min_tokens=GEN)
    if entry == "batch":
        return e.generate_batch(reqs, sp, forced_output_ids=forced)
    return e.generate_continuous(reqs, sp, forced_output_ids=forced, max_live=8, admit_min=1)


def _close(got, want, what):
    worst = 0.0
    for i, (r, w) in enumerate(zip(got, want)):
        assert r["token_ids"] == w["token_ids"]
        assert r["prompt_hidden_states"].shape == w["prompt_hidden_states"].shape, f"{what}: request {i}: prompt_hidden_states is not complete"
        a, b = _rel(r["prompt_hidden_states"], w["prompt_hidden_states"]), _rel(r["hidden_states"], w["hidden_states"])
        assert a < 5e-3 and b < 5e-3, f"{what}: request {i}: prompt_hidden_states {a:.2e}, hidden_states {b:.2e}"
        worst = max(worst, a, b)
    return worst


def _delta(e, before):
    now = e.prefix_cache_stats()
    return {k: now[k] - before[k] for k in now}


@pytest.mark.parametrize("kv", ["auto", "fp8"])
@pytest.mark.parametrize("entry", ["batch", "continuous"])
def test_on_against_off(hip, entry, kv):
    """6 requests share 96 tokens and have tails of 5 .. 40: hits are 5 x 96 on the first call (one leader, five followers) and 6 x 96 on the second (six
    new tails behind the cached prefix); a request repeated verbatim hits ((len - 1) // 16) * 16.  hidden_states and the complete prompt_hidden_states
    within the bound of the run with caching off."""
    on, off = _engine(True, kv=kv), _engine(False, kv=kv)
    assert off.prefix_cache_stats() == {k: 0 for k in on.prefix_cache_stats()}
    first, second = _family(3), _family(3, tails=(7, 9, 17, 31, 16, 38))
    for q, q2 in zip(first, second):
        assert q["prompt_token_ids"][:96] == q2["prompt_token_ids"][:96]
        q2["prompt_token_ids"][96] = (q2["prompt_token_ids"][96] + 1000) % VOCAB      # (other tails than the first call's)
    forced = _forced(6)
    w1 = _close(_run(on, entry, first, forced), _run(off, entry, first, forced), "first call")
    assert on.prefix_cache_stats()["hits"] == 5 * 96 and on.prefix_cache_stats()["queries"] == sum(len(q["prompt_token_ids"]) for q in first)
    s0 = on.prefix_cache_stats()
    w2 = _close(_run(on, entry, second, forced), _run(off, entry, second, forced), "second call")
    assert _delta(on, s0)["hits"] == 6 * 96
    s0 = on.prefix_cache_stats()
    w3 = _close(_run(on, entry, first[3:4], forced[:1]), _run(off, entry, first[3:4], forced[:1]), "verbatim repeat")
    n = len(first[3]["prompt_token_ids"])
    assert _delta(on, s0)["hits"] == ((n - 1) // 16) * 16
    assert off.prefix_cache_stats() == {k: 0 for k in s0}, "with the feature off the statistics stay zero"
    print(f"prefix caching {entry} kv={kv}: worst _rel {max(w1, w2, w3):.2e} (bound 5e-3); stats {on.prefix_cache_stats()}")


def test_inputs_embeds_share_by_identity_only(hip):
    """Equal placeholder ids, different embedding rows, no mm_hash: no sharing, and the result is the uncached one within the bound (a false hit would miss
    it by orders of magnitude).  Equal rows share, through their bytes or through an equal mm_hash."""
    on, off = _engine(True), _engine(False)
    D = on.config.hidden_size
    g = torch.Generator().manual_seed(9)
    ids = [7] * 64 + [11, 12, 13, 14, 15]
    e1, e2 = (torch.randn(69, D, generator=g) * 0.5).bfloat16().cuda(), (torch.randn(69, D, generator=g) * 0.5).bfloat16().cuda()
    pos = on.text_position_ids(69)
    forced = _forced(1)

    def req(e, **kw):
        return {"prompt_token_ids": list(ids), "inputs_embeds": e, "position_ids": pos, **kw}

    _close(_run(on, "batch", [req(e1)], forced), _run(off, "batch", [req(e1)], forced), "first image")
    s0 = on.prefix_cache_stats()
    _close(_run(on, "batch", [req(e2)], forced), _run(off, "batch", [req(e2)], forced), "another image behind the same placeholder ids")
    assert _delta(on, s0)["hits"] == 0, "different embedding rows shared a prefix"
    s0 = on.prefix_cache_stats()
    _close(_run(on, "batch", [req(e1.clone())], forced), _run(off, "batch", [req(e1)], forced), "the first image again, by its bytes")
    assert _delta(on, s0)["hits"] == 64
    on.reset_prefix_cache()
    e3 = e1.clone()
    e3[66:] = e2[66:]      # the same image, another question behind it
    _run(on, "batch", [req(e1, mm_hash="image-1")], forced)
    s0 = on.prefix_cache_stats()
    _close(_run(on, "batch", [req(e3, mm_hash="image-1")], forced), _run(off, "batch", [req(e3)], forced), "equal mm_hash")
    assert _delta(on, s0)["hits"] == 64
    s0 = on.prefix_cache_stats()
    _close(_run(on, "batch", [req(e3, mm_hash="image-2")], forced), _run(off, "batch", [req(e3)], forced), "another mm_hash")
    assert _delta(on, s0)["hits"] == 0


def test_eviction_recomputes(hip):
    """4 slots, 7 distinct prefixes one after the other, then the first again: it was evicted, is recomputed, and the result is within the bound."""
    on, off = _engine(True, slots=4), _engine(False, slots=4)
    forced = _forced(1)
    fams = [_family(20 + i, n=1, shared=48) for i in range(7)]
    for f in fams:
        _run(on, "batch", f, forced)
    s0 = on.prefix_cache_stats()
    assert s0["evictions"] == 3 and s0["hits"] == 0
    _close(_run(on, "batch", fams[0], forced), _run(off, "batch", fams[0], forced), "the first prefix again")
    d = _delta(on, s0)
    assert d["hits"] == 0 and d["evictions"] == 1
    s0 = on.prefix_cache_stats()
    _close(_run(on, "batch", fams[6], forced), _run(off, "batch", fams[6], forced), "the last prefix is still there")
    assert _delta(on, s0)["hits"] == 48


def test_vllm_config_reaches_the_engine(hip):
    from thinkdiff.models.mllama_vllm_generate_1 import MllamaVllmGenerate_1
    from thinkdiff.models.mllama_vllm_t5_embed_decoder_2 import MllamaVllmT5EmbedDecoderForConditionalGeneration_5
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig
    tc = Qwen2VLTextConfig(num_hidden_layers=1, intermediate_size=512, vocab_size=VOCAB, hidden_size=512, num_attention_heads=4, num_key_value_heads=2)
    for on in (True, False):
        vc = {"enable_prefix_caching": on, "max_model_len": 64, "max_num_seqs": 2, "max_num_batched_tokens": 128}
        for m in (MllamaVllmGenerate_1(text_config=tc, vllm_config=vc), MllamaVllmT5EmbedDecoderForConditionalGeneration_5(text_config=tc, vllm_config=vc)):
            assert (m.mllama._prefix_cache is not None) == on
            assert m.mllama.prefix_cache_stats() == {k: 0 for k in ("queries", "hits", "passes", "copies", "copied_rows", "in_place", "deferred", "evictions", "hidden_bytes")}
    m = MllamaVllmGenerate_1(text_config=tc, vllm_config={"max_model_len": 64, "max_num_seqs": 2})
    assert m.mllama._prefix_cache is None, "off by default"
    r = {"prompt_token_ids": [1, 2, 3]}
    m._fill_mm_hash(r, [torch.zeros(2, 2)])
    assert "mm_hash" not in r
    m.mllama.set_prefix_caching(True)
    m._fill_mm_hash(r, [torch.zeros(2, 2)])
    assert isinstance(r["mm_hash"], bytes)
