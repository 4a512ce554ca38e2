"""A stand-in engine for the host logic of n / best_of parallel sampling (tests/test_parallel_sampling_cpu.py), in the manner of
tests/test_scheduler_cpu.py: the engine calls of the three generate entries are replaced by a deterministic toy model on the CPU that CHECKS the
bookkeeping on every call and records it.

  prefill   _prefill_packed_slots (generate_continuous) and forward(want_logits=True) (generate_batch / generate on the lone-prompt path, which the
            stand-in forces with packed_prefill = False and a prefill_rows below two padded prompts): the slot then holds the prompt's tokens;
  fork      _fork_slots: the source must hold EXACTLY a prompt (prefilled, nothing decoded on it yet) of the length the caller names, the
            destinations are distinct, in range, not the source and not live; each then holds the parent's tokens;
  decode    _decode_slots / decode_batch: slots distinct, every slot prefilled or forked (a slot that left the previous step is forgotten, so a
            stale slot shows), the cache length reported for a slot equal to what it holds, positions in step with it.

The toy model's next-token logits are one-hot at (7 t + 3) mod V.  The sampler stub reads the REAL packed TdSampleRow table: at temperature 0 a
row takes the argmax, otherwise argmax + 5 seed + 3 offset + stream (mod V) -- so children with seeds s, s + 1, .. diverge, each reproducibly, and
`expected_tokens` restates a seeded child's tokens without the engine.  The logprobs stub scores token t as -(1 + t mod 7) / 8.
"""
from types import SimpleNamespace

import torch

V, D = 97, 8
KEY = 1      # what the patched _draw_sampler_key returns


def next_token(tok):
    return (int(tok) * 7 + 3) % V


def token_score(tok):
    return -(1 + int(tok) % 7) / 8.0


def expected_tokens(prompt, seed, n_tokens, temperature=1.0):
    """The tokens of a SEEDED sequence (its draws depend on (seed, its own token count) only)."""
    out, t = [], prompt[-1]
    for j in range(n_tokens):
        t = (next_token(t) + (5 * seed + 3 * j if temperature > 0 else 0)) % V
        out.append(t)
    return out


class _History:
    """Stands in for thinkdiff._hip.Sampler (the penalties' token history): logs the resets."""
    handle = 0xBEEF

    def __init__(self, calls):
        self.calls = calls

    def reset_slot(self, slot, prompt_ids=None):
        self.calls.append(["history_reset", int(slot), [int(t) for t in (prompt_ids or [])]])


class _Edits:
    """Stands in for thinkdiff._hip.LogitEdits: keeps each slot's banned set and bias, logs the calls."""
    handle = 0xED17

    def __init__(self, calls):
        self.calls, self.banned, self.bias = calls, {}, {}

    def reset_slot(self, slot):
        self.calls.append(["edit_reset", int(slot)])
        self.banned[slot], self.bias[slot] = set(), {}

    def set_bias(self, slot, bias):
        self.calls.append(["edit_bias", int(slot), sorted(bias)])
        self.bias[slot] = dict(bias)

    def ban(self, slot, ids, on=True):
        self.calls.append(["edit_ban", int(slot), [int(t) for t in ids], bool(on)])
        self.banned[slot] = (self.banned[slot] | set(ids)) if on else (self.banned[slot] - set(ids))

    def allow_only(self, slot, ids):
        self.calls.append(["edit_allow", int(slot), [int(t) for t in ids]])
        self.banned[slot] = set(range(V)) - set(ids)


def fake_engine(n_slots, slot_len=64, prefill_rows=96):
    from thinkdiff import _hip
    from thinkdiff.models import qwen2_vl as Q

    class Fake(Q.Qwen2VLTextEngine):
        packed_prefill = False

        def __init__(self):      # no HIP handle: only what the generate entries touch
            self.config = SimpleNamespace(hidden_size=D, vocab_size=V)
            self.device = torch.device("cpu")
            self.n_slots, self.slot_len, self.prefill_rows = n_slots, slot_len, prefill_rows
            self.cache = {}          # slot -> tokens it holds
            self.fresh = {}          # slot -> True while it holds a prompt and nothing else
            self.last_live = set()
            self.max_rows = 0
            self.prefilled = []      # the prompts, in prefill order
            self.forks = []          # (src, dst slots, length)
            self.calls = []          # every engine call, for the comparison with the parent commit's trace
            self.tables = []         # (seed, stream, slot) per live row of every sample_rows call
            self.history, self.edits = _History(self.calls), _Edits(self.calls)

        def __del__(self):
            pass

        def _sampler_state(self):
            return self.history

        def _logit_edits(self):
            return self.edits

        def embed_tokens(self, token_ids):
            out = torch.zeros(len(token_ids), D, dtype=torch.bfloat16)
            out[:, 0] = torch.tensor(list(token_ids), dtype=torch.float32)
            return out

        def _logits_for(self, tok, row):
            row.zero_()
            row[next_token(tok)] = 8.0

        def _hold(self, slot, toks):
            assert 0 <= slot < self.n_slots      # (a slot handed out while its sequence still decodes shows up as a cache length out of step)
            self.cache[slot], self.fresh[slot] = list(toks), True

        def forward(self, position_ids, token_ids=None, inputs_embeds=None, pos0=0, want_hidden=True, want_logits=False, slot=0):
            toks = token_ids.tolist() if inputs_embeds is None else [int(t) for t in inputs_embeds[:, 0].float().tolist()]
            hid = self.embed_tokens(toks) if inputs_embeds is None else inputs_embeds
            if not want_logits:      # a request with nothing to generate: prompt states through a free slot
                assert 0 <= slot < self.n_slots
                return hid, None
            assert pos0 == 0 and position_ids[0].tolist() == list(range(len(toks)))
            self._hold(slot, toks)
            self.prefilled.append(toks)
            self.calls.append(["forward", slot, len(toks)])
            lg = torch.zeros(V, dtype=torch.bfloat16)
            self._logits_for(toks[-1], lg)
            return hid, lg

        def _prefill_packed_slots(self, k, slots_c, emb, pos, lens_c, hid_out, logits_out):
            slots, lens = list(slots_c), list(lens_c)
            assert len(set(slots)) == k and sum(lens) == emb.shape[0] <= self.prefill_rows and pos.shape == (3, sum(lens))
            self.calls.append(["prefill", slots, lens])
            r = 0
            for b, (s, n) in enumerate(zip(slots, lens)):
                toks = [int(t) for t in emb[r:r + n, 0].float().tolist()]
                assert pos[0, r:r + n].tolist() == list(range(n))
                self._hold(s, toks)
                self.prefilled.append(toks)
                hid_out[r:r + n] = emb[r:r + n]
                self._logits_for(toks[-1], logits_out[b])
                r += n

        def _fork_slots(self, src, dst_slots, length):
            dst = [int(d) for d in dst_slots]
            assert self.fresh.get(int(src)), f"fork from slot {src}, which holds no untouched prompt"
            assert len(self.cache[int(src)]) == int(length), "the fork's length is not the parent's prompt length"
            assert dst and len(set(dst)) == len(dst) and int(src) not in dst
            self.forks.append((int(src), dst, int(length)))
            self.calls.append(["fork", int(src), dst, int(length)])
            for d in dst:
                self._hold(d, self.cache[int(src)])

        def _step(self, slots, toks, cache_pos, pos_rows, hid_out, logits_out):
            n = len(slots)
            for s in self.last_live - set(slots):      # a sequence that left the step gave its slot back
                self.cache.pop(s, None)
            assert len(set(slots)) == n and all(s in self.cache for s in slots), "a decode row names a slot that was neither prefilled nor forked, or a repeated one"
            self.last_live = set(slots)
            self.max_rows = max(self.max_rows, n)
            self.calls.append(["decode", list(slots), [int(t) for t in toks]])
            for i, s in enumerate(slots):
                assert int(cache_pos[i]) == len(self.cache[s]) < self.slot_len, "cache length out of step with the slot's contents"
                assert [int(p[i]) for p in pos_rows] == [len(self.cache[s])] * 3
                t = int(toks[i])
                self.cache[s].append(t)
                self.fresh[s] = False
                hid_out[i].zero_()
                hid_out[i, 0], hid_out[i, 1] = float(t), float(s)
                self._logits_for(t, logits_out[i])

        def _decode_slots(self, n, slots_np, tok_dev, pos_dev, cache_np, hid_out, logits_out):
            self._step([int(x) for x in slots_np[:n]], tok_dev[:n].tolist(), cache_np, pos_dev, hid_out, logits_out)

        def decode_batch(self, token_ids, position_ids, cache_pos, want_logits=True, slots=None):
            n = len(cache_pos)
            hid, lg = torch.zeros(n, D, dtype=torch.bfloat16), torch.zeros(n, V, dtype=torch.bfloat16)
            pos = torch.as_tensor(position_ids)
            self._step([int(s) for s in (slots if slots is not None else range(n))], [int(t) for t in token_ids], cache_pos, pos, hid, lg)
            return hid, lg

    e = Fake()

    def rows_of(table):
        arr = (_hip.TdSampleRow * table.shape[0]).from_buffer_copy(table.contiguous().numpy().tobytes())
        return [(int(a.seed), int(a.stream), int(a.slot), float(a.temperature)) for a in arr]

    def sample_top_p(logits, temperature, top_p, key, step):
        logits = logits.reshape(-1, V)      # (the op takes one row as [vocab] too)
        e.calls.append(["sample_top_p", logits.shape[0], int(step)])
        return logits.float().argmax(dim=1).to(torch.int32)

    def sample_rows(logits, params, offsets, state, update_state):
        rows = rows_of(params)
        assert len(rows) == logits.shape[0] == offsets.numel()
        e.tables.append([r[:3] for r in rows])
        e.calls.append(["sample_rows", [list(r[:2]) for r in rows], offsets.tolist()])
        top = logits.float().argmax(dim=1).tolist()
        return torch.tensor([(t + (5 * seed + 3 * int(o) + stream if temp > 0 else 0)) % V
                             for t, (seed, stream, _, temp), o in zip(top, rows, offsets.tolist())], dtype=torch.int32)

    def sample_rows_edit(logits, params, offsets, state, update_state, edits, edit_slots):
        rows = rows_of(params)
        assert edits == _Edits.handle and len(rows) == logits.shape[0] == offsets.numel() == edit_slots.numel()
        e.calls.append(["sample_rows_edit", [list(r[:2]) for r in rows], offsets.tolist(), edit_slots.tolist()])
        z = logits.float().clone()
        for i, s in enumerate(edit_slots.tolist()):
            if s >= 0:
                for t, b in e.edits.bias[s].items():
                    z[i, t] += b
                if e.edits.banned[s]:
                    z[i, sorted(e.edits.banned[s])] = float("-inf")
        return torch.tensor([(t + (5 * seed + 3 * int(o) + stream if temp > 0 else 0)) % V
                             for t, (seed, stream, _, temp), o in zip(z.argmax(dim=1).tolist(), rows, offsets.tolist())], dtype=torch.int32)

    def logprobs_rows(logits, ids, n_top, top_cap):
        n = logits.shape[0]
        e.calls.append(["logprobs_rows", n_top.tolist(), int(top_cap)])
        lp = torch.tensor([token_score(t) for t in ids.tolist()], dtype=torch.float32)
        return lp, torch.ones(n, dtype=torch.int32), torch.full((n, top_cap), -1, dtype=torch.int32), torch.full((n, top_cap), float("-inf"))

    ops = SimpleNamespace(sample_top_p=sample_top_p, sample_rows=sample_rows, sample_rows_edit=sample_rows_edit, logprobs_rows=logprobs_rows)
    return e, Q, ops


def patch(monkeypatch, Q, ops):
    monkeypatch.setattr(Q, "_OPS", ops)
    monkeypatch.setattr(Q.Qwen2VLTextEngine, "_draw_sampler_key", staticmethod(lambda generator=None: KEY))


def prompts(n, seed=5, lo=1, hi=8):
    g = torch.Generator().manual_seed(seed)
    return [{"prompt_token_ids": torch.randint(0, V, (lo + (3 * i) % (hi - lo + 1),), generator=g).tolist()} for i in range(n)]


def n1_scenarios(extra):
    """Three calls with one sequence per request, as (name, run(e, Q) -> results): what tests/golden/parallel_sampling_n1_calls.json records of the
    commit before n / best_of existed (extra = {}) and the test replays with n = 1 spelled out (extra = {"n": 1} / {"n": 1, "best_of": 1})."""
    reqs = prompts(11)

    def top_p(e, Q):
        return e.generate_continuous(reqs, Q.SamplingParams(temperature=0.0, max_tokens=6, min_tokens=2, ignore_eos=False, stop_token_ids=[4, 9, 30], **extra),
                                     eos_token_id=5, max_live=4, admit_min=1)

    def rows(e, Q):
        sps = [Q.SamplingParams(temperature=1.0, seed=40 + i if i % 3 else None, max_tokens=3 + i % 4, min_tokens=1, logprobs=0 if i % 4 == 0 else None, **extra)
               for i in range(len(reqs))]
        return e.generate_continuous(iter([reqs[:5], reqs[5:]]), sps, max_live=3, admit_min=2)

    def batch(e, Q):
        sps = [Q.SamplingParams(temperature=1.0, seed=7 * i, max_tokens=2 + i % 3, min_tokens=1, **extra) for i in range(6)]
        return e.generate_batch(reqs[:6], sps)

    return [("continuous_top_p", top_p), ("continuous_rows", rows), ("batch_rows", batch)]


def run_n1_trace(extra):
    """-> {scenario: {"calls": the engine calls, "token_ids": per request}} on fresh stand-in engines (sampler key patched by the caller)."""
    out = {}
    for name, run in n1_scenarios(extra):
        e, Q, _ = fake_engine(n_slots=8, slot_len=32, prefill_rows=8)
        res = run(e, Q)
        out[name] = {"calls": e.calls, "token_ids": [r["token_ids"] for r in res]}
    return out


# ---- the decode entries, call for call ----------------------------------------------------------------------------------------------------------
def entry_scenarios():
    """The calls tests/golden/decode_entries_calls.json records of the commit before the three generate loops were folded onto one token source, one
    prompt prefill and one live-row table: (name, engine keywords, run(e, Q) -> results) on the stand-in above, and two beam searches on
    beam_search_common.fake_engine (engine keywords with "beam": True).  Prompts of 1..8 tokens and prefill_rows = 8 throughout."""
    reqs = prompts(11)
    six = reqs[:6]
    std = dict(n_slots=8, slot_len=32, prefill_rows=8)
    p0 = six[2]["prompt_token_ids"]
    t1 = next_token(p0[-1])
    t2, t3 = next_token(t1), next_token(next_token(t1))
    firsts = [next_token(r["prompt_token_ids"][-1]) for r in reqs]      # request i's first token at temperature 0
    out = []

    def add(name, run, **kw):
        out.append((name, {**std, **kw}, run))

    # generate
    add("generate_top_p", lambda e, Q: e.generate(p0, Q.SamplingParams(temperature=0.0, max_tokens=5, min_tokens=5)))
    add("generate_rows_seed_penalty", lambda e, Q: e.generate(p0, Q.SamplingParams(temperature=1.0, seed=3, repetition_penalty=1.2, max_tokens=4, min_tokens=1)))
    add("generate_forced_short", lambda e, Q: e.generate(p0, Q.SamplingParams(max_tokens=5, min_tokens=5), forced_output_ids=[5, 6, 7]))
    add("generate_forced_long", lambda e, Q: e.generate(p0, Q.SamplingParams(max_tokens=4, min_tokens=4, logprobs=0), forced_output_ids=[5, 6, 7, 8, 9, 10]))
    add("generate_logprobs", lambda e, Q: e.generate(p0, Q.SamplingParams(temperature=0.0, max_tokens=3, min_tokens=3, logprobs=1)))
    add("generate_stop_around_min_tokens", lambda e, Q: e.generate(p0, Q.SamplingParams(temperature=0.0, max_tokens=6, min_tokens=2, stop_token_ids=[t1, t3])))
    add("generate_eos", lambda e, Q: e.generate(p0, Q.SamplingParams(temperature=0.0, max_tokens=6, min_tokens=1, ignore_eos=False), eos_token_id=t2))
    add("generate_n3", lambda e, Q: e.generate(p0, Q.SamplingParams(temperature=1.0, seed=11, n=3, max_tokens=3, min_tokens=1)))

    # generate_batch, 6 requests
    add("batch_top_p_eos_stops", lambda e, Q: e.generate_batch(six, Q.SamplingParams(
        temperature=0.0, max_tokens=6, min_tokens=2, ignore_eos=False, stop_token_ids=[next_token(firsts[1]), next_token(next_token(firsts[3])), firsts[4]]),
        eos_token_id=next_token(next_token(next_token(firsts[0])))))
    add("batch_list_seeds_budgets_logprobs", lambda e, Q: e.generate_batch(six, [
        Q.SamplingParams(temperature=1.0, seed=7 * i if i % 2 else None, max_tokens=i % 5, min_tokens=1, logprobs=1 if i % 3 == 0 else None) for i in range(6)]))
    add("batch_forced", lambda e, Q: e.generate_batch(six, Q.SamplingParams(max_tokens=3, min_tokens=3),
                                                      forced_output_ids=[[(10 * i + j) % V for j in range(i)] for i in range(6)]))
    add("batch_mixed_n_best_of", lambda e, Q: e.generate_batch(six, [
        Q.SamplingParams(temperature=1.0, seed=30 + i if i != 4 else None, max_tokens=2 + i % 3, min_tokens=1, n=(1, 3, 1, 2, 1, 1)[i], best_of=4 if i == 3 else None)
        for i in range(6)]), n_slots=12)
    add("batch_bad_words_and_bias", lambda e, Q: e.generate_batch(six, [
        Q.SamplingParams(temperature=0.0, max_tokens=4, min_tokens=4, bad_words_token_ids=[[firsts[0], next_token(firsts[0])]] if i == 0 else None,
                         logit_bias={5: 100.0} if i == 1 else None) for i in range(6)]))
    add("batch_reaches_slot_len", lambda e, Q: e.generate_batch(six, Q.SamplingParams(temperature=0.0, max_tokens=6, min_tokens=6)), slot_len=10)

    # generate_continuous, 11 requests
    for name, run in n1_scenarios({}):
        add("n1_" + name, run)
    add("continuous_mixed_n_chunks", lambda e, Q: e.generate_continuous(iter([reqs[:4], reqs[4:9], reqs[9:]]), [
        Q.SamplingParams(temperature=1.0, seed=20 + i if i % 4 else None, max_tokens=2 + i % 3, min_tokens=1, n=(1, 3, 2)[i % 3] if i % 4 != 3 else 1,
                         best_of=2 if i % 4 == 3 else None) for i in range(11)], max_live=4, admit_min=2))
    add("continuous_forced_with_empty", lambda e, Q: e.generate_continuous(reqs, Q.SamplingParams(max_tokens=13, min_tokens=13),
                                                                            forced_output_ids=[[(10 * i + j) % V for j in range((2 * i) % 5)] for i in range(11)],
                                                                            max_live=3, admit_min=1))
    add("continuous_best_of_3", lambda e, Q: e.generate_continuous(reqs, Q.SamplingParams(temperature=1.0, seed=9, n=1, best_of=3, max_tokens=4, min_tokens=1),
                                                                    max_live=7, admit_min=1))
    add("continuous_list_logprobs", lambda e, Q: e.generate_continuous(reqs, [
        Q.SamplingParams(temperature=0.0 if i % 4 == 0 else 1.0, logprobs=i % 3 if i % 2 else None, max_tokens=2 + i % 4, min_tokens=1, ignore_eos=bool(i % 3),
                         stop_token_ids=[next_token(firsts[i])] if i % 4 == 0 else None) for i in range(11)], eos_token_id=4, max_live=5, admit_min=2))

    # beam_search
    bp = [[1, 2, 3], [4, 5, 6, 7, 0, 9, 10], [8]]
    out.append(("beam_r3_w2_eos", dict(beam=True, n_slots=6, slot_len=32, prefill_rows=8),
                lambda e, Q: e.beam_search([{"prompt_token_ids": p} for p in bp], Q.BeamSearchParams(beam_width=2, max_tokens=4), eos_token_id=3)))
    out.append(("beam_r1_w3_ignore_eos", dict(beam=True, n_slots=3, slot_len=32, prefill_rows=8),
                lambda e, Q: e.beam_search([{"prompt_token_ids": bp[1]}], Q.BeamSearchParams(beam_width=3, max_tokens=5, ignore_eos=True), eos_token_id=3)))
    return out


def _summary(res):
    """What a scenario's record keeps of the results: token ids, and per output the token ids and the cumulative logprob where present."""
    out = []
    for r in (res if isinstance(res, list) else [res]):
        d = {"token_ids": [int(t) for t in r["token_ids"]]}
        if "cumulative_logprob" in r:
            d["cumulative_logprob"] = float(r["cumulative_logprob"])
        if "outputs" in r:
            d["outputs"] = [{k: ([int(t) for t in o[k]] if k == "token_ids" else float(o[k])) for k in ("token_ids", "cumulative_logprob") if k in o} for o in r["outputs"]]
        out.append(d)
    return out


def run_entries_trace(set_ops):
    """-> {scenario: {"calls": the stand-in's call log, "results": _summary}} on fresh stand-in engines.  set_ops(Q, ops) puts the stand-in's ops in
    place of torch.ops.thinkdiff_hip; the sampler key is patched by the caller, as for run_n1_trace."""
    import json

    import beam_search_common as B
    out = {}
    for name, kw, run in entry_scenarios():
        kw = dict(kw)
        e, Q, ops = (B.fake_engine if kw.pop("beam", False) else fake_engine)(**kw)
        set_ops(Q, ops)
        out[name] = json.loads(json.dumps({"calls": e.calls, "results": _summary(run(e, Q))}))
    return out


if __name__ == "__main__":      # python tests/parallel_sampling_common.py OUT.json: how tests/golden/decode_entries_calls.json was written, at the parent commit
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thinkdiff-mlre_amd"))
    from thinkdiff.models import qwen2_vl as _Q
    _Q.Qwen2VLTextEngine._draw_sampler_key = staticmethod(lambda generator=None: KEY)
    with open(sys.argv[1], "w") as fh:
        json.dump(run_entries_trace(lambda Q, ops: setattr(Q, "_OPS", ops)), fh, separators=(",", ":"))
        fh.write("\n")
