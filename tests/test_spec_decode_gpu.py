"""Speculative decoding on the GPU: the engine's verify step against stepping one token at a time (T3) and the generate loop end to end (T4).

Tiny engines throughout: 2 layers at the two decoder widths (hidden 1536 with 12 / 2 heads, hidden 3584 with 28 / 4), random weights from one seed,
short cache slots.  Bound between two schedules of one model: the project's _rel < 5e-3 (tests/test_qwen2_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"2b": dict(hidden_size=1536, num_attention_heads=12, num_key_value_heads=2), "7b": dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4)}
MODES = {"bf16": {}, "kv_fp8": dict(kv="fp8"), "w_fp8": dict(quant="fp8"), "w_mxfp4": dict(quant="mxfp4")}
VOCAB = 2048

# T4's margin, MEASURED, not chosen: on the parent commit, the largest difference of one token's logprob between two existing schedules of the same
# forced sequences -- `generate` one request at a time against `generate_batch`, as test_batched_decode_equals_one_sequence_at_a_time runs them, on the
# engine, weights (seed 11) and requests of test_loop_end_to_end, top-5 logprobs of all 96 positions -- was 0.00785 (hidden 1536) and 0.00784 (hidden
# 3584): one bf16 step of a logit near 1.  x 4: two logits move, and each moves both ways.  Compared the way _agree compares, those two schedules
# disagree in rank 1 on 0 (1536) and 1 (3584) of the 96 positions, inside the cap of 1 in 8.  (DESIGN.md 5.20 holds the same figures.)
MARGIN_MEASURED = 0.00785
MARGIN = 4 * MARGIN_MEASURED


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def _weights(shape, seed):
    """The oracle's tiny decoder at one of the two widths (oracle/qwen2vl_ref.py: norm weights around 1, embeddings 0.5), its Linears drawn at
    0.02 sqrt(512 / hidden): the gain per layer of the project's tiny config (hidden 512, std 0.02), for which the bound between two schedules was
    set.  At std 0.02 a Linear of width 3584 has 2.6 x that gain, and the PARENT's own two schedules (generate against generate_batch on forced ids)
    already sit at 6.8 - 7.1e-3 on this model, above the bound with none of the code under test involved; scaled, they sit at 1.3 - 1.8e-3
    (measured on the MI355X for weight seeds 7, 8, 9 at both widths)."""
    from oracle import qwen2vl_ref as Q
    d = SHAPES[shape]
    cfg = Q.tiny_config(hidden=d["hidden_size"], num_heads=d["num_attention_heads"], num_kv_heads=d["num_key_value_heads"], intermediate=2048, vocab=VOCAB)
    return Q.init_weights(cfg, seed=seed, std=0.02 * (512 / d["hidden_size"]) ** 0.5)


def _engine(shape, mode, max_len=1024, slots=8, seed=7):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    m = MODES[mode]
    cfg = Qwen2VLTextConfig(num_hidden_layers=2, intermediate_size=2048, vocab_size=VOCAB, **SHAPES[shape])
    e = Qwen2VLTextEngine(cfg, max_model_len=max_len, kv_cache_dtype=m.get("kv", "auto"))
    e.load_state_dict(_weights(shape, seed))
    if m.get("quant"):
        e.quantize_weights(m["quant"])
    e.set_slots(slots)
    return e


def _prefill(e, prompts, slots):
    for p, s in zip(prompts, slots):
        e.forward(e.text_position_ids(len(p)), torch.tensor(p, dtype=torch.int32), slot=s, want_hidden=False)


def _step_alone(e, slots, pos, toks):
    """Sequence b decodes toks[b] one step at a time (every step serves the sequences that still have a token) -> per sequence (hidden, logits)."""
    hid, lg = [[] for _ in slots], [[] for _ in slots]
    for j in range(max(len(t) for t in toks)):
        on = [b for b in range(len(slots)) if len(toks[b]) > j]
        h, l = e.decode_batch([toks[b][j] for b in on], [[pos[b] + j for b in on]] * 3, [pos[b] + j for b in on], slots=[slots[b] for b in on])
        for i, b in enumerate(on):
            hid[b].append(h[i].clone())
            lg[b].append(l[i].clone())
    return [torch.stack(h) for h in hid], [torch.stack(l) for l in lg]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_verify_equals_stepping_one_token_at_a_time(hip, shape, mode):
    g = torch.Generator().manual_seed(3)
    lens, slots, n_new = [9, 33, 17, 40, 5], [4, 0, 6, 1, 3], [3, 1, 8, 2, 5]
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in lens]
    A, B = _engine(shape, mode), _engine(shape, mode)
    _prefill(A, prompts, slots)
    _prefill(B, prompts, slots)
    # every n_new == 1: the plain step's bits
    t1 = torch.randint(0, VOCAB, (5,), generator=g).tolist()
    ha, la = A.verify_batch(t1, [lens] * 3, lens, [1] * 5, slots=slots)
    hb, lb = B.decode_batch(t1, [lens] * 3, lens, slots=slots)
    assert torch.equal(ha, hb) and torch.equal(la, lb)
    pos = [n + 1 for n in lens]
    # forced tokens, n_new = [3, 1, 8, 2, 5]
    toks = [torch.randint(0, VOCAB, (k,), generator=g).tolist() for k in n_new]
    flat = [t for ts in toks for t in ts]
    fpos = [p + j for p, ts in zip(pos, toks) for j in range(len(ts))]
    # the same step twice -- it writes the same cache rows both times -- first with the multi-row attention kernel forced (the automatic routing takes the
    # row form for a step with 8 rows in it), then as routed: both against stepping
    prev = hip.lib().td_attention_verify_set_form(2)
    try:
        hm, lm = A.verify_batch(flat, [fpos] * 3, pos, n_new, slots=slots)
        torch.cuda.synchronize()
    finally:
        hip.lib().td_attention_verify_set_form(prev)
    hv, lv = A.verify_batch(flat, [fpos] * 3, pos, n_new, slots=slots)
    hs, ls = _step_alone(B, slots, pos, toks)
    torch.cuda.synchronize()
    r0 = 0
    for b, k in enumerate(n_new):
        eh, el = _rel(hv[r0:r0 + k], hs[b]), _rel(lv[r0:r0 + k], ls[b])
        assert eh < 5e-3 and el < 5e-3, f"sequence {b} ({k} rows): hidden {eh:.2e}, logits {el:.2e}"
        eh, el = _rel(hm[r0:r0 + k], hs[b]), _rel(lm[r0:r0 + k], ls[b])
        assert eh < 5e-3 and el < 5e-3, f"sequence {b} ({k} rows), multi-row kernel: hidden {eh:.2e}, logits {el:.2e}"
        for layer in range(2):
            ek = _rel(A.read_kv(layer, slots[b], pos[b], k), B.read_kv(layer, slots[b], pos[b], k))
            assert ek < 5e-3, f"sequence {b}, layer {layer}: new cache rows {ek:.2e}"
        r0 += k
    # stale rows: sequence 2 fed 8 rows above; keep ONE (advance by 1), then decode on.  B, which stepped, forgets 7 of its 8 the same way: its rows past
    # pos + 1 are overwritten by what follows, exactly as A's rejected rows are
    nxt = torch.randint(0, VOCAB, (4,), generator=g).tolist()
    p2, s2 = pos[2] + 1, slots[2]
    C = _engine(shape, mode)      # never saw the drafts
    _prefill(C, [prompts[2]], [s2])
    C.decode_batch([t1[2]], [[lens[2]]] * 3, [lens[2]], slots=[s2])
    C.decode_batch([toks[2][0]], [[pos[2]]] * 3, [pos[2]], slots=[s2])
    for j, t in enumerate(nxt):
        ha, _ = A.decode_batch([t], [[p2 + j]] * 3, [p2 + j], slots=[s2])
        hc, _ = C.decode_batch([t], [[p2 + j]] * 3, [p2 + j], slots=[s2])
        assert _rel(ha, hc) < 5e-3, f"step {j} after a verify whose drafts were dropped"


def test_verify_takes_the_wide_path_beyond_64_rows(hip):
    """16 sequences x 8 rows = 128 rows: the step's Linears are the split-K tile kernels (decode_step's `wide`)."""
    g = torch.Generator().manual_seed(5)
    A, B = _engine("2b", "bf16", max_len=1024, slots=16), _engine("2b", "bf16", max_len=1024, slots=16)
    lens = [5 + (3 * i) % 11 for i in range(16)]
    slots = list(range(15, -1, -1))
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in lens]
    _prefill(A, prompts, slots)
    _prefill(B, prompts, slots)
    toks = [torch.randint(0, VOCAB, (8,), generator=g).tolist() for _ in range(16)]
    flat = [t for ts in toks for t in ts]
    fpos = [p + j for p in lens for j in range(8)]
    hv, lv = A.verify_batch(flat, [fpos] * 3, lens, [8] * 16, slots=slots)
    hs, ls = _step_alone(B, slots, lens, toks)
    for b in range(16):
        assert _rel(hv[8 * b:8 * b + 8], hs[b]) < 5e-3 and _rel(lv[8 * b:8 * b + 8], ls[b]) < 5e-3


def test_verify_refusals(hip):
    e = _engine("2b", "bf16", max_len=256, slots=4)      # slots of 64 rows
    ok = dict(token_ids=[1, 2, 3], position_ids=[[5, 6, 7]] * 3, cache_pos=[5, 9], n_new=[2, 1])
    with pytest.raises(hip.ThinkDiffHipError, match="n_new"):
        e.verify_batch([1] * 9, [[0] * 9] * 3, [5], [9])
    with pytest.raises(hip.ThinkDiffHipError, match="n_new"):
        e.verify_batch([1], [[0]] * 3, [5, 6], [0, 1])
    with pytest.raises(hip.ThinkDiffHipError, match="slot capacity"):
        e.verify_batch([1] * 4, [[0] * 4] * 3, [61], [4])
    with pytest.raises(hip.ThinkDiffHipError, match="more than one"):
        e.verify_batch(ok["token_ids"], ok["position_ids"], ok["cache_pos"], ok["n_new"], slots=[2, 2])
    with pytest.raises(hip.ThinkDiffHipError, match="batch 5"):
        e.verify_batch([1] * 5, [[0] * 5] * 3, [1] * 5, [1] * 5)


# ---- T4: the loop end to end -----------------------------------------------------------------------------------------------------------------------
class ReplayDraft:
    """Guesses what a previous run produced: the sequence whose prompt the history starts with."""

    def __init__(self, prompts, outputs):
        self.seqs = [list(p) + list(o) for p, o in zip(prompts, outputs)]
        self.n_prompt = [len(p) for p in prompts]

    def propose(self, token_ids, k):
        ids = list(token_ids)
        for s, n in zip(self.seqs, self.n_prompt):
            if ids[:n] == s[:n]:
                return np.array(s[len(ids):len(ids) + k], dtype=np.int32)
        return np.empty(0, dtype=np.int32)


def _requests():
    g = torch.Generator().manual_seed(17)
    out = []
    for n in (12, 30, 7, 21):      # each prompt repeats a stretch of itself: something for prompt lookup to find
        ids = torch.randint(0, VOCAB, (n,), generator=g).tolist()
        out.append({"prompt_token_ids": ids + ids[:5]})
    return out


def _agree(e, reqs, spec, what):
    """The speculative run's tokens and hidden states against the plain path replayed on those tokens (forced ids, logprobs = 1)."""
    from thinkdiff.models.qwen2_vl import SamplingParams
    forced = [r["token_ids"] for r in spec]
    rep = e.generate_batch(reqs, SamplingParams(max_tokens=24, min_tokens=24, logprobs=1), forced_output_ids=forced)
    by_margin = total = 0
    for i, (s, r) in enumerate(zip(spec, rep)):
        assert len(s["token_ids"]) == 24 and s["hidden_states"].shape == r["hidden_states"].shape
        assert _rel(s["hidden_states"], r["hidden_states"]) < 5e-3, f"{what}: request {i}"
        for tok, d in zip(s["token_ids"], r["logprobs"]):
            total += 1
            top = max(v.logprob for v in d.values())
            if d[tok].rank != 1 and d[tok].logprob < top:      # (a tie with the best token is the best token)
                assert top - d[tok].logprob <= MARGIN, f"{what}: request {i} chose a token {top - d[tok].logprob:.4f} below the plain path's best (margin {MARGIN})"
                by_margin += 1
    print(f"{what}: {by_margin} of {total} positions pass by the margin")
    assert by_margin * 8 <= total, f"{what}: {by_margin} of {total} positions pass by the margin only"


def _redraw(hip, e, reqs, run, sps):
    """How many tokens of `run` the plain path draws on their own prefix: request i's tokens are fed one decode step at a time, and token g is drawn
    by td_sample_rows_bf16 at (seed_i, g, 0) from the logits in front of it (the prefill's for g = 0)."""
    hit = 0
    for i, (q, r, sp) in enumerate(zip(reqs, run, sps)):
        p, toks = q["prompt_token_ids"], r["token_ids"]
        _, lg0 = e.forward(e.text_position_ids(len(p)), torch.tensor(p, dtype=torch.int32), slot=i, want_hidden=False, want_logits=True)
        _, lgs = _step_alone(e, [i], [len(p)], [toks[:-1]])
        logits = torch.cat([lg0.reshape(1, -1), lgs[0]])
        rec = dict(temperature=sp.temperature, top_p=sp.top_p, min_p=sp.min_p, top_k=sp.top_k, slot=-1, stream=0, seed=sp.seed)
        drawn = hip.sample_rows(logits, [rec] * len(toks), list(range(len(toks)))).cpu().tolist()
        hit += sum(a == b for a, b in zip(drawn, toks))
    return hit


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_loop_end_to_end(hip, shape):
    from thinkdiff.models.qwen2_vl import SamplingParams, SpeculativeConfig
    e = _engine(shape, "bf16", max_len=1024, slots=8, seed=11)
    reqs = _requests()
    greedy = SamplingParams(temperature=0.0, max_tokens=24, min_tokens=24)
    plain = e.generate_batch(reqs, greedy)
    ngram = e.generate_batch(reqs, greedy, speculative=SpeculativeConfig(num_speculative_tokens=4, prompt_lookup_max=3, prompt_lookup_min=1))
    st_n = e.spec_stats()
    _agree(e, reqs, ngram, "n-gram")
    replay = e.generate_continuous(reqs, greedy, speculative=ReplayDraft([r["prompt_token_ids"] for r in reqs], [r["token_ids"] for r in plain]), max_live=3, admit_min=1)
    st_r = e.spec_stats()
    _agree(e, reqs, replay, "replay")
    print(f"n-gram {st_n}, replay {st_r}")
    assert st_r["accepted"] > 0 and st_r["steps"] < 24 * 2 and st_r["emitted"] == 96
    assert st_n["emitted"] == 96
    # seeded, temperature 1.  A seeded request draws token number g at (seed, g, 0), so every speculative token must be what the PLAIN path draws on the
    # same prefix: the tokens are fed one step at a time through decode_batch (the plain step), and td_sample_rows_bf16 draws at (seed, g) from each
    # step's logits (_redraw).  Position by position on one prefix: a sequence-level comparison says nothing past the first differing draw, because the
    # contexts differ from there.  A wrong draw offset on any row of the verify step fails nearly every position (1 hit in 2048 by chance).
    # The bound is the plain path's own: its seeded generate_batch run -- the parent's code, none of the code under test -- scored the same way does NOT
    # reproduce every position either, because an inverse-CDF draw over near-tied bf16 logits lands on a neighbouring token when a logit moves by one
    # bf16 step between two schedules: measured on the MI355X, 86 of 96 (hidden 1536) and 85 of 96 (hidden 3584).  With m misses of 96 on the plain
    # run, the speculative run, whose logits differ from the replay's by another schedule of the same kind, is allowed m + 3 sqrt(m (1 - m / 96)):
    # the same miss rate and three binomial standard deviations.  Measured: 84 of 96 (1536) and 82 of 96 (3584), against bounds of 77 and 76.  The
    # cap of 1 position in 8 that the greedy rule uses is NOT met at 3584 (82 < 84); the plain run meets it by one or two positions.
    seeded = [SamplingParams(temperature=1.0, seed=100 + i, max_tokens=24, min_tokens=24) for i in range(4)]
    plain_s = e.generate_batch(reqs, seeded)
    spec_s = e.generate_batch(reqs, seeded, speculative=ReplayDraft([r["prompt_token_ids"] for r in reqs], [r["token_ids"] for r in plain_s]))
    st_s = e.spec_stats()
    assert st_s["emitted"] == 96 and st_s["accepted"] > 0
    hit_plain, hit_spec = _redraw(hip, e, reqs, plain_s, seeded), _redraw(hip, e, reqs, spec_s, seeded)
    m = max(96 - hit_plain, 1)
    floor = 96 - (m + 3.0 * (m * (1.0 - m / 96.0)) ** 0.5)
    print(f"seeded: the plain path's draw on the token's own prefix reproduces {hit_plain} of 96 plain and {hit_spec} of 96 speculative tokens (floor {floor:.1f}); {st_s}")
    assert hit_plain * 2 >= 96, "the plain run itself is not reproduced: the replay is broken, not the speculative loop"
    assert hit_spec >= floor, f"seeded: only {hit_spec} of 96 speculative tokens are the plain path's draw at (seed, token number) on their own prefix (floor {floor:.1f})"
    assert all(s["token_ids"][0] == p["token_ids"][0] for s, p in zip(spec_s, plain_s)), "token 0 is drawn from the same prefill logits under the same key"
    rep = e.generate_batch(reqs, SamplingParams(max_tokens=24, min_tokens=24), forced_output_ids=[r["token_ids"] for r in spec_s])
    for i, (s, r) in enumerate(zip(spec_s, rep)):
        assert _rel(s["hidden_states"], r["hidden_states"]) < 5e-3, f"seeded: request {i}"
