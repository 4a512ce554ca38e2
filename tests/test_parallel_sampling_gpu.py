"""n / best_of parallel sampling on the GPU: the tiny decoder of tests/test_logit_edits_gpu.py (hidden 512, 2 layers, 4 / 2 heads, vocab 4096) with 8
cache slots.  One prefill, a KV fork, and k sequences that draw from seeds s, s + 1, ..: greedy children agree bit for bit, seeded runs repeat,
best_of returns the most probable of the same children, penalties and bad words act per child, generate_continuous returns what generate_batch
returns, and a model class passes vllm_config["best_of"] through.  Every comparison is an equality."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 4096
PROMPT = list(range(5, 25))
OTHER = list(range(40, 57))


@pytest.fixture(scope="module")
def engine(hip):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    return Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                               intermediate_size=1024, vocab_size=V), max_model_len=256, n_slots=8).init_random(3, std=0.05)


def _sp(**kw):
    from thinkdiff.models.qwen2_vl import SamplingParams
    return SamplingParams(**{**dict(max_tokens=12, min_tokens=12), **kw})


def test_greedy_children_are_bit_identical(hip, engine):
    o = engine.generate(PROMPT, _sp(temperature=0.0, n=3))
    outs = o["outputs"]
    assert len(outs) == 3 and [c["index"] for c in outs] == [0, 1, 2] and len(outs[0]["token_ids"]) == 12
    assert outs[0]["token_ids"] == outs[1]["token_ids"] == outs[2]["token_ids"]
    assert torch.equal(outs[0]["hidden_states"], outs[1]["hidden_states"]) and torch.equal(outs[0]["hidden_states"], outs[2]["hidden_states"])
    assert o["token_ids"] == outs[0]["token_ids"] and torch.equal(o["hidden_states"], outs[0]["hidden_states"]) and o["prompt_hidden_states"].shape == (20, 512)
    assert "logprobs" not in o and "cumulative_logprob" not in o


@pytest.fixture(scope="module")
def seeded4(engine):
    """temperature 1, seed 7, n = 4 with logprobs = 0 (child i draws from seed 7 + i): what best_of = 4 is compared against."""
    return engine.generate(PROMPT, _sp(temperature=1.0, top_p=1.0, seed=7, n=4, logprobs=0))


@pytest.fixture(scope="module")
def seeded3(engine):
    return engine.generate(PROMPT, _sp(temperature=1.0, top_p=1.0, seed=7, n=3))


def test_seeded_children_differ_and_repeat(hip, engine, seeded3):
    b = engine.generate(PROMPT, _sp(temperature=1.0, top_p=1.0, seed=7, n=3))
    ta, tb = [c["token_ids"] for c in seeded3["outputs"]], [c["token_ids"] for c in b["outputs"]]
    assert ta == tb and all(torch.equal(x["hidden_states"], y["hidden_states"]) for x, y in zip(seeded3["outputs"], b["outputs"])), "a seeded call repeats exactly"
    top1 = engine.generate(PROMPT, _sp(temperature=1.0, top_p=1.0, seed=7, logprobs=1, max_tokens=1, min_tokens=1))["logprobs"][0]
    assert not (ta[0] == ta[1] == ta[2]), f"three equal lists from seeds 7, 8, 9 (top-1 logprob of the first token {max(v.logprob for v in top1.values()):.3f})"
    assert all(len(t) == 12 for t in ta) and torch.equal(seeded3["hidden_states"], seeded3["outputs"][0]["hidden_states"])


def test_best_of_returns_the_best_children_in_order(hip, engine, seeded4):
    o = engine.generate(PROMPT, _sp(temperature=1.0, top_p=1.0, seed=7, n=2, best_of=4))
    kids = seeded4["outputs"]
    order = sorted(range(4), key=lambda j: (-kids[j]["cumulative_logprob"], j))[:2]
    assert len(o["outputs"]) == 2 and [c["index"] for c in o["outputs"]] == [0, 1]
    for c, j in zip(o["outputs"], order):
        assert c["token_ids"] == kids[j]["token_ids"] and c["cumulative_logprob"] == kids[j]["cumulative_logprob"] and "logprobs" not in c
        assert torch.equal(c["hidden_states"], kids[j]["hidden_states"])
    assert o["outputs"][0]["cumulative_logprob"] >= o["outputs"][1]["cumulative_logprob"]
    assert o["token_ids"] == kids[order[0]]["token_ids"] and "logprobs" not in o and o["cumulative_logprob"] == kids[order[0]]["cumulative_logprob"]
    assert all(len(c["logprobs"]) == 12 for c in kids), "the n = 4 run asked for logprobs and has them"
    assert len({tuple(c["token_ids"]) for c in kids}) > 1


def test_a_two_token_bad_word_acts_on_each_childs_own_output(hip, engine, seeded3):
    """The word is two consecutive tokens of child 1's output, the first of which child 1 had not written before.  With the word banned, the same
    three seeds on the same three rows: child 1 is unchanged up to the word's first token and takes another token behind it; a sibling that never
    wrote the pair is unchanged to the last token -- the ban of one child's plan does not reach the others -- and nobody writes the pair."""
    T = [c["token_ids"] for c in seeded3["outputs"]]
    s = next(i for i in range(1, 10) if T[1][i] not in T[1][:i])
    word = T[1][s:s + 2]
    o = engine.generate(PROMPT, _sp(temperature=1.0, top_p=1.0, seed=7, n=3, bad_words_token_ids=[word]))
    out = [c["token_ids"] for c in o["outputs"]]
    assert out[1][:s + 1] == T[1][:s + 1] and out[1][s + 1] != T[1][s + 1], (s, word, out[1], T[1])
    for c in range(3):
        assert len(out[c]) == 12 and all(out[c][j:j + 2] != word for j in range(11))
        if all(T[c][j:j + 2] != word for j in range(11)):
            assert out[c] == T[c], f"child {c} never wrote the word and is unchanged"


def test_penalties_keep_one_history_per_child(hip, engine):
    """With a penalty on, child i's generated-token counts live in the history slot of ITS cache slot (generate: slots 0, 1, 2): after the call each
    slot holds exactly the histogram of that child's tokens, and the prompt mask of every child is the shared prompt's."""
    o = engine.generate(PROMPT, _sp(temperature=1.0, top_p=1.0, seed=7, n=3, frequency_penalty=1.5, presence_penalty=0.5, repetition_penalty=1.2))
    out = [c["token_ids"] for c in o["outputs"]]
    assert len({tuple(t) for t in out}) > 1 and all(len(t) == 12 for t in out)
    st = engine._sampler_state()
    for slot, t in enumerate(out):
        assert torch.equal(st.read_counts(slot).cpu().long(), torch.bincount(torch.tensor(t), minlength=V)), f"history slot {slot} is child {slot}'s"
        assert torch.equal(st.read_prompt_mask(slot).cpu().long(), torch.bincount(torch.tensor(PROMPT), minlength=V).clamp(max=1))
    again = engine.generate(PROMPT, _sp(temperature=1.0, top_p=1.0, seed=7, n=3, frequency_penalty=1.5, presence_penalty=0.5, repetition_penalty=1.2))
    assert [c["token_ids"] for c in again["outputs"]] == out, "a reused slot starts its history over"


def test_continuous_returns_what_the_batch_returns(hip, engine):
    """n = 2 next to n = 1 on 4 slots.  The four sequences fit at once, so both entries make the same launches -- one packed prefill of the three
    prompts, the fork, decode steps over the same rows in the same order, rows leaving at the same steps -- and every token agrees, the unseeded
    request's too.  (Across DIFFERENT prefill passes tokens are not compared: a prompt's cache rows depend on its place in a packed pass by a bf16
    step -- DESIGN.md 5.14 and 5.16 -- and a draw next to a boundary then moves to the neighbouring token.)  Then six requests on the same four slots, where the
    second n = 2 request has to wait: every sequence arrives complete."""
    reqs = [{"prompt_token_ids": PROMPT}, {"prompt_token_ids": OTHER}, {"prompt_token_ids": PROMPT[:9]}]
    sps = [_sp(temperature=1.0, top_p=1.0, seed=11, n=2, max_tokens=9, min_tokens=9), _sp(temperature=1.0, max_tokens=5, min_tokens=5),
           _sp(temperature=0.8, seed=31, max_tokens=7, min_tokens=7)]
    batch = engine.generate_batch(reqs, sps, generator=torch.Generator().manual_seed(3))
    cont = engine.generate_continuous(reqs, sps, max_live=4, admit_min=1, generator=torch.Generator().manual_seed(3))
    for r, sp, b, c in zip(reqs, sps, batch, cont):
        assert ("outputs" in b) == ("outputs" in c) == (sp.width > 1) and len(c.get("outputs", [c])) == sp.n
        assert torch.equal(b["prompt_hidden_states"], c["prompt_hidden_states"]) and c["prompt_hidden_states"].shape == (len(r["prompt_token_ids"]), 512)
        for x, y in zip(b.get("outputs", [b]), c.get("outputs", [c])):
            assert x["token_ids"] == y["token_ids"] and len(x["token_ids"]) == sp.max_tokens
            assert torch.equal(x["hidden_states"], y["hidden_states"])
    assert cont[0]["outputs"][0]["token_ids"] != cont[0]["outputs"][1]["token_ids"]
    more = reqs + [{"prompt_token_ids": OTHER[:11]}, {"prompt_token_ids": PROMPT[:13]}, {"prompt_token_ids": OTHER[:6]}]
    sps2 = sps + [_sp(temperature=1.0, seed=41, n=2, best_of=3, max_tokens=6, min_tokens=6), _sp(temperature=1.0, seed=51, max_tokens=4, min_tokens=4),
                  _sp(temperature=1.0, seed=61, n=2, max_tokens=3, min_tokens=3)]
    out = engine.generate_continuous(more, sps2, max_live=4, admit_min=1)
    for r, sp, o in zip(more, sps2, out):
        kids = o.get("outputs", [o])
        assert len(kids) == sp.n and all(len(c["token_ids"]) == sp.max_tokens and c["hidden_states"].shape == (sp.max_tokens, 512) for c in kids)
        assert o["prompt_hidden_states"].shape == (len(r["prompt_token_ids"]), 512) and ("cumulative_logprob" in o) == (sp.width > sp.n)
    again = engine.generate_continuous(more, sps2, max_live=4, admit_min=1)
    assert [o["token_ids"] for o, sp in zip(again, sps2) if sp.seed is not None] == [o["token_ids"] for o, sp in zip(out, sps2) if sp.seed is not None]


def test_refusals_on_the_engine(hip, engine):
    with pytest.raises(hip.ThinkDiffHipError, match="needs 9 cache slots"):
        engine.generate(PROMPT, _sp(n=9))
    with pytest.raises(ValueError, match="forced_output_ids"):
        engine.generate(PROMPT, _sp(n=2), forced_output_ids=[1, 2, 3])


def test_model_class_passes_best_of_through(hip):
    from thinkdiff.models.mllama_vllm_generate_1 import MllamaVllmGenerate_1
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig
    tc = Qwen2VLTextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=1024, vocab_size=V)
    prompts = [PROMPT, OTHER, PROMPT[:9]]
    vc = {"max_model_len": 64, "max_num_seqs": 4, "max_tokens": 6, "min_tokens": 6, "ignore_eos": True, "temperature": 1.0, "top_p": 1.0, "seed": 5}

    def run(extra):
        m = MllamaVllmGenerate_1(tc, vllm_config={**vc, **extra}, request_builder=lambda samples, i: {"prompt_token_ids": samples["answers"][i]})
        m.mllama.init_random(3, std=0.05)
        forks = []
        fork = m.mllama._fork_slots
        m.mllama._fork_slots = lambda src, dst, n: (forks.append((src, list(dst), n)), fork(src, dst, n))[1]
        out = m.forward_inner({"answers": prompts}, generator=torch.Generator().manual_seed(0))
        return m, forks, out["generated_token"]["output_token_ids"]

    m, forks, toks = run({"best_of": 2})
    assert (m.mllama_sampling_params.n, m.mllama_sampling_params.best_of, m.mllama_sampling_params.width) == (1, 2, 2)
    assert [len(d) for _, d, _ in forks] == [1, 1, 1] and [n for _, _, n in forks] == [20, 17, 9], "one fork per request, at its prompt length"
    assert all(len(t) == 6 for t in toks)
    _, forks1, toks1 = run({})
    assert forks1 == [] and all(len(t) == 6 for t in toks1)
    # output 0 of best_of = 2 is the more probable of the children seeded 5 and 6, through the engine entry and chunks the model used
    import dataclasses
    e, sp = m.mllama, dataclasses.replace(m.mllama_sampling_params, n=2, best_of=None, logprobs=0)
    got = []
    for chunk in (prompts[:2], prompts[2:]):
        for o in e.generate_batch([{"prompt_token_ids": p} for p in chunk], sp):
            got.append(tuple(max(o["outputs"], key=lambda c: (c["cumulative_logprob"], -c["index"]))["token_ids"]))
    assert got == [tuple(t) for t in toks]
