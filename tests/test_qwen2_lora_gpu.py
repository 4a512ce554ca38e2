"""Per-request LoRA on the Qwen2-VL decode engine, end to end on the tiny decoder (oracle.qwen2vl_ref.tiny_config: hidden 512, 2 layers, intermediate 1024,
vocab 320): every sequence against the oracle run on ITS OWN merged weights W + s B A (tests/qwen2_lora_common.merged_state_dict), in float32 (ref32) and in
bf16 (ref16), under the engine bounds of tests/test_qwen2_gpu.py: e16 < 2e-2, e32 < 1.5 rel(ref16, ref32) + 2e-3, logits < 3e-2.

So that the bound cannot hide a missing adapter, every adapter used moves the oracle's hidden states by rel(merged, base) >= 0.2, ten times the bound, and
test_adapters_move_the_oracle asserts it.  Adapters: a (rank 16) and b (rank 64) on all seven Linears, c on q_proj + v_proj only at rank 5 (r_pad 16), its B
drawn at 0.1 N(0, 1) to reach that effect through two Linears."""
import functools
import json
import os

import pytest
import torch

import qwen2_lora_common as C
from oracle import qwen2vl_ref as Q

pytestmark = pytest.mark.gpu

CFG = Q.tiny_config()
SD = Q.init_weights(CFG, seed=41)
SPECS = {"a": dict(rank=16, seed=1), "b": dict(rank=64, seed=2), "c": dict(rank=5, seed=3, modules=("self_attn.q_proj", "self_attn.v_proj"), b_std=0.1)}
IDS = {"a": 1, "b": 2, "c": 3}


def _rel(a, b):
    return C.rel_rmse(a, b)


@functools.lru_cache(maxsize=None)
def adapter(name):
    return C.make_adapter(CFG, **SPECS[name])


@functools.lru_cache(maxsize=None)
def weights(name, f32, w8=False):
    """The oracle's weights under adapter `name` (None: the base model), merged in float64 and rounded once."""
    sd = SD
    if w8:
        import qwen2_w8_common as W
        lin = tuple(m.split(".")[-1] + ".weight" for m in C.MODULES)
        sd = {k: (W.quantize_rows(v)[2].to(v.dtype) if (k.endswith(lin) or k == "lm_head.weight") else v) for k, v in SD.items()}
    dt = torch.float32 if f32 else torch.bfloat16
    if name is None:
        return {k: v.to(dt) for k, v in sd.items()}
    return C.merged_state_dict(sd, *adapter(name), dtype=dt)


def request(name):
    from thinkdiff.models.qwen2_vl import LoRARequest
    return None if name is None else LoRARequest(name, IDS[name])


def check(got, name, tokens, what, pos=None, logits=None, w8=False, hidden_fn=None):
    """Hidden states of one sequence against the oracle on its adapter's merged weights."""
    tokens = torch.as_tensor(tokens).long()
    pos = Q.text_position_ids(tokens.numel()) if pos is None else pos
    run = hidden_fn or (lambda sd: Q.text_model_hidden(sd, CFG, pos, token_ids=tokens)[0])
    ref16, ref32 = run(weights(name, False, w8)), run(weights(name, True, w8))
    e16, e32, eref = _rel(got, ref16), _rel(got, ref32), _rel(ref16, ref32)
    assert e16 < 2e-2 and e32 < 1.5 * eref + 2e-3, f"{what} under {name}: hip~bf16 {e16:.4f}, hip~fp32 {e32:.4f}, bf16~fp32 {eref:.4f}"
    if logits is not None:
        assert _rel(logits, Q.lm_logits(weights(name, False, w8), CFG, ref16[-1])) < 3e-2, f"{what} under {name}: logits"
    return e32


def engine(n_slots=8, max_len=96, lora=True, max_loras=3, names=("a", "b", "c"), **kw):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    e = Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=CFG.hidden, num_hidden_layers=CFG.num_layers, num_attention_heads=CFG.num_heads,
                                            num_key_value_heads=CFG.num_kv_heads, intermediate_size=CFG.intermediate, vocab_size=CFG.vocab,
                                            tie_word_embeddings=CFG.tie_embeddings), max_model_len=max_len, n_slots=n_slots, prefill_rows=1024,
                          **(dict(enable_lora=True, max_loras=max_loras, max_lora_rank=64) if lora else {}), **kw)
    e.load_state_dict(SD)
    for n in names if lora else ():
        e.add_lora(request(n), *adapter(n))
    return e


@pytest.fixture(scope="module")
def eng(hip):
    return engine()


def prompts(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, CFG.vocab, (n,), generator=g).tolist() for n in lens]


def test_adapters_move_the_oracle():
    ids = torch.tensor(prompts([40], 5)[0])
    pos = Q.text_position_ids(40)
    base = Q.text_model_hidden(weights(None, True), CFG, pos, token_ids=ids)[0]
    for name in SPECS:
        moved = _rel(Q.text_model_hidden(weights(name, True), CFG, pos, token_ids=ids)[0], base)
        print(f"adapter {name}: rel(merged, base) = {moved:.3f}")
        assert moved >= 0.2, (name, moved)


def test_prefill_forward_and_packed(eng):
    ids = prompts([40], 5)[0]
    hid, lg = eng.forward(Q.text_position_ids(40), torch.tensor(ids, dtype=torch.int32), want_logits=True, lora_request=request("a"))
    check(hid, "a", ids, "forward", logits=lg)
    names, ps = ["a", "b", None, "a", "c"], prompts([21, 7, 16, 33, 12], 6)
    rows = [{"position_ids": Q.text_position_ids(len(p)), "token_ids": p, "lora_request": request(n)} for p, n in zip(ps, names)]
    hids, lgs = eng.prefill_packed(rows, [4, 0, 2, 1, 3], [0] * 5)
    for h, l, p, n in zip(hids, lgs, ps, names):
        check(h, n, p, "packed prefill", logits=l)      # (the adapter-less prompt is held against the base oracle)


def test_decode_stream_path_with_a_changing_assignment(eng):
    """6 requests of different lengths: the batch shrinks, the LoRA step is captured and replayed; the second call replays the captured steps under
    another row -> adapter assignment."""
    from thinkdiff.models.qwen2_vl import SamplingParams
    ps, forced = prompts([9, 14, 5, 11, 8, 17], 7), prompts([2, 3, 4, 8, 8, 8], 8)
    n0 = eng.lora_info()["launches"]
    for names in (["a", "b", None, "a", "c", None], ["b", None, "c", "c", "a", "b"]):
        reqs = [{"prompt_token_ids": p, "lora_request": request(n)} for p, n in zip(ps, names)]
        out = eng.generate_batch(reqs, SamplingParams(max_tokens=8, min_tokens=8), forced_output_ids=forced)
        for o, p, f, n in zip(out, ps, forced, names):
            assert o["token_ids"] == f
            check(torch.cat([o["prompt_hidden_states"], o["hidden_states"]]), n, p + f, "generate_batch")
    assert eng.lora_info()["launches"] > n0


def test_decode_wide_path(hip):
    """70 sequences for 2 steps: the split-K step with its RMSNorm in a launch of its own."""
    from thinkdiff.models.qwen2_vl import SamplingParams
    e = engine(n_slots=72, max_len=24)
    B = 70
    names = [("a", "b", None, "c")[i % 4] for i in range(B)]
    ps, forced = prompts([3 + (5 * i) % 9 for i in range(B)], 9), prompts([2] * B, 10)
    reqs = [{"prompt_token_ids": p, "lora_request": request(n)} for p, n in zip(ps, names)]
    out = e.generate_batch(reqs, SamplingParams(max_tokens=2, min_tokens=2), forced_output_ids=forced)
    for i in range(0, B, 3):
        check(torch.cat([out[i]["prompt_hidden_states"], out[i]["hidden_states"]]), names[i], ps[i] + forced[i], f"wide step, sequence {i}")


def test_adapterless_calls_return_the_old_bits(eng):
    from thinkdiff.models.qwen2_vl import SamplingParams
    plain = engine(lora=False)
    ps = prompts([9, 14, 5], 11)
    sp = SamplingParams(temperature=0.8, top_p=0.9, seed=5, max_tokens=6, min_tokens=6)
    before = eng.lora_info()["launches"]
    a = eng.generate_batch([{"prompt_token_ids": p} for p in ps], sp)
    b = plain.generate_batch([{"prompt_token_ids": p} for p in ps], sp)
    assert eng.lora_info()["launches"] == before, "an adapter-less call enqueued a low-rank launch"
    assert eng.lora_info()["resident"] == 3 and plain.lora_info()["max_loras"] == 0
    for x, y in zip(a, b):
        assert x["token_ids"] == y["token_ids"] and torch.equal(x["hidden_states"], y["hidden_states"]) and torch.equal(x["prompt_hidden_states"], y["prompt_hidden_states"])
    with pytest.raises(ValueError, match="enable_lora"):
        plain.generate_batch([{"prompt_token_ids": ps[0], "lora_request": request("a")}], sp)


def test_children_and_beams_inherit_the_adapter(eng):
    from thinkdiff.models.qwen2_vl import BeamSearchParams, SamplingParams
    p = prompts([12], 12)[0]
    kw = dict(temperature=1.0, top_p=1.0, max_tokens=6, min_tokens=6, ignore_eos=True)
    two = eng.generate(p, SamplingParams(n=2, seed=21, **kw), lora_request=request("a"))
    base = eng.generate(p, SamplingParams(seed=21, **kw))
    for j in range(2):
        one = eng.generate(p, SamplingParams(seed=21 + j, **kw), lora_request=request("a"))
        assert two["outputs"][j]["token_ids"] == one["token_ids"], f"child {j} of n = 2 under an adapter"
        check(torch.cat([one["prompt_hidden_states"], two["outputs"][j]["hidden_states"]]), "a", p + one["token_ids"], f"child {j}")
    assert base["token_ids"] != two["outputs"][0]["token_ids"], "the adapter changes what is sampled under seed 21"
    ps, names = prompts([10, 15], 13), ["b", "c"]
    bp = BeamSearchParams(beam_width=2, max_tokens=4, ignore_eos=True)
    reqs = [{"prompt_token_ids": q, "lora_request": request(n)} for q, n in zip(ps, names)]
    both = eng.beam_search(reqs, bp)
    for r, q, n, got in zip(reqs, ps, names, both):
        alone = eng.beam_search([r], bp)[0]
        assert [o["token_ids"] for o in got["outputs"]] == [o["token_ids"] for o in alone["outputs"]], f"beams under {n}"
        for o in got["outputs"]:
            check(torch.cat([got["prompt_hidden_states"], o["hidden_states"]]), n, q + o["token_ids"], f"beam under {n}")


def test_speculative_run_returns_the_plain_tokens(eng):
    """The rule tests/test_spec_decode_gpu.py applies to adapter-less runs: the speculative run replayed on the plain path (forced ids)."""
    from test_spec_decode_gpu import _agree
    from thinkdiff.models.qwen2_vl import SamplingParams, SpeculativeConfig
    g = torch.Generator().manual_seed(17)
    reqs = []
    for n, name in zip((12, 20, 7, 16), ("a", "b", None, "c")):
        ids = torch.randint(0, CFG.vocab, (n,), generator=g).tolist()
        reqs.append({"prompt_token_ids": ids + ids[:5], "lora_request": request(name)})
    spec = eng.generate_batch(reqs, SamplingParams(temperature=0.0, max_tokens=24, min_tokens=24),
                              speculative=SpeculativeConfig(num_speculative_tokens=4, prompt_lookup_max=3, prompt_lookup_min=1))
    assert eng.spec_stats()["emitted"] == 96
    _agree(eng, reqs, spec, "n-gram under adapters")


def test_prefix_caching_is_salted_by_the_adapter(hip):
    from test_prefix_cache_gpu import _close
    from thinkdiff.models.qwen2_vl import SamplingParams
    on, off = engine(names=("a", "b"), enable_prefix_caching=True), engine(names=("a", "b"))
    p, forced = prompts([50], 14)[0], prompts([4], 15)
    sp = SamplingParams(max_tokens=4, min_tokens=4)
    want = {n: off.generate_batch([{"prompt_token_ids": p, "lora_request": request(n)}], sp, forced_output_ids=forced) for n in ("a", "b")}
    hits = []
    for n in ("a", "b", "a"):
        s0 = on.prefix_cache_stats()["hits"]
        got = on.generate_batch([{"prompt_token_ids": p, "lora_request": request(n)}], sp, forced_output_ids=forced)
        hits.append(on.prefix_cache_stats()["hits"] - s0)
        _close(got, want[n], f"prefix caching under {n}")
        check(torch.cat([got[0]["prompt_hidden_states"], got[0]["hidden_states"]]), n, p + forced[0], "prefix caching")
    assert hits == [0, 0, 48], hits      # a then b: no hit; a again: its three whole blocks


@pytest.mark.parametrize("mode", ["w8", "kv8"])
def test_composition_with_fp8_weights_and_fp8_cache(hip, mode):
    from thinkdiff.models.qwen2_vl import SamplingParams
    import qwen2_kv8_common as K
    e = engine(names=("a",), **({"kv_cache_dtype": "fp8"} if mode == "kv8" else {}))
    if mode == "w8":
        e.quantize_weights("fp8")
    p, f = prompts([18], 16)[0], prompts([5], 17)[0]
    n0 = e.weight_stream_launches()
    o = e.generate_batch([{"prompt_token_ids": p, "lora_request": request("a")}, {"prompt_token_ids": p}], SamplingParams(max_tokens=5, min_tokens=5),
                         forced_output_ids=[f, f])
    toks = torch.tensor(p + f)
    fn = (lambda sd: K.text_model_hidden(sd, CFG, Q.text_position_ids(23), token_ids=toks, kv_round=K.kv_round)[0]) if mode == "kv8" else None
    for r, n in zip(o, ("a", None)):
        check(torch.cat([r["prompt_hidden_states"], r["hidden_states"]]), n, p + f, mode, w8=mode == "w8", hidden_fn=fn)
    if mode == "w8":
        assert e.weight_stream_launches() > n0, "the base Linears of a LoRA step still read the 8-bit copy"


def test_pool_replaces_the_least_recently_used(hip, tmp_path):
    from safetensors.torch import save_file
    from thinkdiff.models.qwen2_vl import LoRARequest, SamplingParams
    e = engine(max_loras=2, names=("a", "b", "c"))
    p, f = prompts([10], 18)[0], prompts([3], 19)
    sp = SamplingParams(max_tokens=3, min_tokens=3)
    run = lambda req: e.generate_batch([{"prompt_token_ids": p, "lora_request": req}], sp, forced_output_ids=f)[0]
    first = {n: run(request(n)) for n in ("a", "b", "c")}      # c takes the place of a, the least recently used
    assert e.lora_info()["evictions"] == 1 and e.lora_info()["resident"] == 2 and sorted(e._lora.resident) == [2, 3]
    again = run(request("a"))                                     # ... and a comes back with the bits it had
    assert torch.equal(again["hidden_states"], first["a"]["hidden_states"]) and torch.equal(again["prompt_hidden_states"], first["a"]["prompt_hidden_states"])
    assert sorted(e._lora.resident) == [1, 3] and e.list_loras() == [1, 2, 3]
    with pytest.raises(ValueError, match="max_loras=2"):
        e.generate_batch([{"prompt_token_ids": p, "lora_request": request(n)} for n in ("a", "b", "c")], sp)
    assert e.remove_lora(1) and e.list_loras() == [2, 3]
    with pytest.raises(ValueError, match="lora_path"):
        run(request("a"))
    sd, cfg = adapter("a")
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(tmp_path, "adapter_model.safetensors"))
    with open(os.path.join(tmp_path, "adapter_config.json"), "w") as fh:
        json.dump(cfg, fh)
    disk = run(LoRARequest("a-from-disk", 7, str(tmp_path)))      # loaded at its first use
    assert torch.equal(disk["hidden_states"], first["a"]["hidden_states"]) and 7 in e.list_loras()


@pytest.mark.parametrize("cls", ["embed", "generate"])
def test_vllm_config_reaches_the_engine_on_both_model_classes(hip, cls):
    from oracle import aligner_ref as A
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig
    tc = Qwen2VLTextConfig(hidden_size=CFG.hidden, num_hidden_layers=CFG.num_layers, num_attention_heads=CFG.num_heads, num_key_value_heads=CFG.num_kv_heads,
                           intermediate_size=CFG.intermediate, vocab_size=CFG.vocab)
    vc = {"max_model_len": 64, "max_tokens": 4, "min_tokens": 4, "enable_lora": True, "max_loras": 2, "max_lora_rank": 16,
          "lora_request": {"lora_name": "a", "lora_int_id": 1}}
    if cls == "generate":
        from thinkdiff.models.mllama_vllm_generate_1 import MllamaVllmGenerate_1
        m = MllamaVllmGenerate_1(tc, vllm_config=vc, request_builder=lambda s, i: {"prompt_token_ids": s["ids"][i]})
        assert m.mllama.lora_info()["max_loras"] == 2 and m.mllama._lora.max_lora_rank == 16
        assert [r["lora_request"].lora_int_id for r in m._requests({"ids": [[1, 2], [3]]}, [0, 1])] == [1, 1]
        return
    from thinkdiff.models.mllama_vllm_t5_embed_decoder_2 import MllamaVllmT5EmbedDecoderForConditionalGeneration_5
    asd = A.init_weights(CFG.hidden, 4096, seed=4)
    p, f = prompts([20], 20)[0], prompts([4], 21)[0]

    def aligner(h):
        lin = torch.nn.functional.linear
        y = lin(torch.nn.functional.gelu(lin(h, asd["mm_projector.0.weight"], asd["mm_projector.0.bias"])), asd["mm_projector.2.weight"], asd["mm_projector.2.bias"])
        return A.t5_layer_norm(y.float(), asd["mm_projector.3.weight"].float()).bfloat16()

    embs = {}
    for name, conf in (("a", vc), (None, {k: v for k, v in vc.items() if k != "lora_request"})):
        m = MllamaVllmT5EmbedDecoderForConditionalGeneration_5(tc, vllm_config=conf)
        m.mllama.load_state_dict(SD)
        m.load_state_dict(asd)
        m.mllama.add_lora(request("a"), *adapter("a"))
        embs[name] = m.get_embed([{"prompt_token_ids": p}], embedding_type="both", need_process=False, forced_output_ids=[f])[0][0]
        ref_h = Q.text_model_hidden(weights(name, False), CFG, Q.text_position_ids(24), token_ids=torch.tensor(p + f))[0]
        assert _rel(embs[name], aligner(ref_h)) < 3e-2, name
    assert _rel(embs["a"], embs[None]) >= 0.2, "get_embed under the configured adapter moves by the adapter's effect"
