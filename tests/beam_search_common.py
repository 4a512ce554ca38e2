"""Shared by tests/test_beam_search_cpu.py and tests/test_beam_search_gpu.py.

  select_ref     a numpy restatement of td_beam_select's rule and placement as include/thinkdiff_hip.h states them (np.float32 adds);
  fake_engine    a stand-in engine for the host logic of Qwen2VLTextEngine.beam_search, in the manner of parallel_sampling_common.fake_engine: the
                 engine calls are replaced by a toy LM on the CPU (vocab 12) that CHECKS the bookkeeping on every call -- a slot decodes only what it
                 holds, the cache length the host names is the slot's, a gather never writes a slot it reads -- and records what every slot held
                 after every step.  A decode row's hidden state encodes (token fed, row, step, cache length before the token);
  brute_force    an independent beam search in Python lists, a transcription of vLLM's LLM.beam_search loop: no rows, no placement, no logs.  It adds
                 in np.float32, as the engine does (vLLM adds Python floats: DESIGN.md 5.17).
"""
import contextlib
from types import SimpleNamespace

import numpy as np
import torch

V, D = 12, 8
NEG_INF = np.float32(-np.inf)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------
def select_ref(top_ids, top_lp, cum_in, rank_in, W, n_in, eos):
    """-> dict of the seven outputs, [R*W] numpy arrays."""
    top_ids, top_lp = np.asarray(top_ids), np.asarray(top_lp, dtype=np.float32)
    cum_in, rank_in = np.asarray(cum_in, dtype=np.float32), np.asarray(rank_in)
    N = cum_in.shape[0]
    out = {"token": np.full(N, -1, np.int32), "cum_out": np.full(N, NEG_INF, np.float32), "rank_out": np.zeros(N, np.int32),
           "copy_src": np.full(N, -1, np.int32), "parent": np.arange(N, dtype=np.int32), "fin_flag": np.zeros(N, np.int32),
           "fin_cum": np.full(N, NEG_INF, np.float32)}
    for base in range(0, N, W):
        cands = []
        for j in range(n_in):
            for c in range(2 * W):
                tid = int(top_ids[base + j, c])
                with np.errstate(invalid="ignore"):
                    cum = np.float32(cum_in[base + j]) + np.float32(top_lp[base + j, c])
                if np.isnan(cum):
                    cum = NEG_INF
                if tid < 0:
                    continue
                if eos >= 0 and tid == eos:
                    if not out["fin_flag"][base + j]:
                        out["fin_flag"][base + j], out["fin_cum"][base + j] = 1, cum
                    continue
                cands.append((cum, int(rank_in[base + j]), c, j, tid))
        cands.sort(key=lambda x: (-float(x[0]), x[1], x[2], x[3]))
        beams = cands[:W]
        row_of, claimed = [None] * W, [False] * W
        for k, b in enumerate(beams):      # a beam whose parent's row is not yet claimed takes it
            if not claimed[b[3]]:
                claimed[b[3]], row_of[k] = True, b[3]
        free = [p for p in range(W) if not claimed[p]]
        for k in range(W):                 # the others (and the missing ones) take the unclaimed rows in ascending order
            if k >= len(beams) or row_of[k] is None:
                row_of[k] = free.pop(0)
        for k in range(W):
            row = base + row_of[k]
            out["rank_out"][row] = k
            if k < len(beams):
                cum, _, _, j, tid = beams[k]
                out["token"][row], out["cum_out"][row], out["parent"][row] = tid, cum, base + j
                out["copy_src"][row] = -1 if j == row_of[k] else base + j
    return out


OUT_KEYS = ("token", "cum_out", "rank_out", "copy_src", "parent", "fin_flag", "fin_cum")


def make_case(rng, R, W, n_in, cap):
    """Inputs of one select launch with what the rule has to get right: few distinct values (ties in cum across rows and columns), -inf logprobs,
    id -1 padding, an EOS id that falls inside the 2 W columns of some rows and only outside them (cap > 2 W) in others, and now and then a request with
    fewer than W candidates.  -> (top_ids, top_lp, cum_in, rank_in, eos)."""
    N = R * W
    top_lp = -rng.integers(0, 6, size=(N, cap)).astype(np.float32) / 4
    top_lp[rng.random((N, cap)) < 0.1] = -np.inf
    top_ids = rng.integers(0, 30, size=(N, cap)).astype(np.int32)
    top_ids[rng.random((N, cap)) < 0.15] = -1
    eos = int(rng.integers(0, 30)) if rng.random() < 0.7 else -1
    if eos >= 0 and cap > 2 * W:
        top_ids[::2, 2 * W:] = eos      # beyond the 2 W columns: not a finisher
        top_ids[::2, :2 * W][top_ids[::2, :2 * W] == eos] = 29 - eos if 29 - eos != eos else 0
    if rng.random() < 0.3:      # the first request has fewer than W candidates
        top_ids[:W, :] = -1
        top_ids[0, :int(rng.integers(0, 2 * W))] = 3
    cum_in = -rng.integers(0, 4, size=N).astype(np.float32) / 2
    rank_in = np.concatenate([rng.permutation(W) for _ in range(R)]).astype(np.int32)
    return top_ids, top_lp, cum_in, rank_in, eos


# ---- the toy LM ----------------------------------------------------------------------------------------------------------------------------------
def toy_logits(seq):
    """bf16 [V]: half-integer scores with ties among the 12 tokens, a function of the whole sequence (two beams never share a row of logits by
    accident, the same prefix always gives the same row)."""
    h = 0
    for i, t in enumerate(seq):
        h = (h * 31 + 7 * int(t) + i) % 1009
    return torch.tensor([((h + 3 * t * t + 5 * t * len(seq)) % 11) / 2.0 for t in range(V)], dtype=torch.float32).bfloat16()


def toy_logprobs(seq):
    """fp32 [V] raw logprobs of the row, and the ids of the whole row in the kernel's order (value descending, id ascending)."""
    lp = torch.log_softmax(toy_logits(seq).float(), dim=0).numpy().astype(np.float32)
    return lp, sorted(range(V), key=lambda t: (-float(lp[t]), t))


def brute_force(prompt, W, T, eos, ignore_eos, length_penalty, keep_all=False):
    """vLLM's loop.  -> the W best (tokens, cumulative logprob, score, finished), best first (keep_all: every completed sequence and live beam)."""
    beams, completed = [([], np.float32(0.0))], []
    for _ in range(T):
        new = []
        for toks, cum in beams:
            lp, order = toy_logprobs(list(prompt) + toks)
            for t in order[:2 * W]:
                c = np.float32(cum) + np.float32(lp[t])
                if eos is not None and t == eos and not ignore_eos:
                    completed.append((toks + [t], c, True))
                else:
                    new.append((toks + [t], c, False))
        beams = [(t, c) for t, c, _ in sorted(new, key=lambda b: -float(b[1]))[:W]]      # (a stable sort: ties keep beam order, then column order)
    completed.extend((t, c, False) for t, c in beams)

    def score(t, c):
        n = len(prompt) + len(t) - (1 if eos is not None and t[-1] == eos else 0)
        return float(c) / (float(n) ** float(length_penalty))
    best = sorted(completed, key=lambda b: -score(b[0], b[1]))[:len(completed) if keep_all else W]
    return [(t, float(c), score(t, c), f) for t, c, f in best]


# ---- the stand-in engine -------------------------------------------------------------------------------------------------------------------------
DOWNLOADS = ("cpu", "tolist", "item", "numpy", "__int__", "__float__", "__bool__", "__index__")


def fake_engine(n_slots, slot_len=32, prefill_rows=64):
    from thinkdiff.models import qwen2_vl as Q

    class Fake(Q.Qwen2VLTextEngine):
        def __init__(self):      # no HIP handle: only what beam_search touches
            self.config = SimpleNamespace(hidden_size=D, vocab_size=V)
            self.device = torch.device("cpu")
            self.n_slots, self.slot_len, self.prefill_rows = n_slots, slot_len, prefill_rows
            self.cache = {}            # slot -> the tokens it holds
            self.calls = []
            self.held = []             # per decode step: {slot: tokens after the step}
            self.downloads = 0         # tensor -> host conversions made by the code under test
            self.in_loop = None        # the count at the loop's first call
            self.loop_downloads = 0    # conversions between the loop's first call and its last
            self._own = 0

        def __del__(self):
            pass

        @contextlib.contextmanager
        def own(self):
            """The stand-in's own reads of tensors are not the engine's downloads."""
            self._own += 1
            try:
                yield
            finally:
                self._own -= 1

        def count(self):
            if not self._own:
                self.downloads += 1

        def mark(self):
            """Called by every op of the loop: whatever was downloaded since the loop's first call came before the loop's end."""
            if self.in_loop is None:
                self.in_loop = self.downloads
            self.loop_downloads = self.downloads - self.in_loop

        def embed_tokens(self, token_ids):
            out = torch.zeros(len(token_ids), D, dtype=torch.bfloat16)
            out[:, 0] = torch.tensor(list(token_ids), dtype=torch.float32)
            return out

        def forward(self, position_ids, token_ids=None, inputs_embeds=None, pos0=0, want_hidden=True, want_logits=False, slot=0):
            with self.own():
                toks = token_ids.tolist()
                assert inputs_embeds is None and pos0 == 0 and want_logits and 0 <= slot < self.n_slots and position_ids[0].tolist() == list(range(len(toks)))
            self.cache[slot] = list(toks)
            self.calls.append(["forward", slot, len(toks)])
            return self.embed_tokens(toks), toy_logits(toks)

        def _prefill_packed_slots(self, k, slots_c, emb, pos, lens_c, hid_out, logits_out):
            slots, lens = list(slots_c), list(lens_c)
            assert len(set(slots)) == k and sum(lens) == emb.shape[0] <= self.prefill_rows and pos.shape == (3, sum(lens))
            self.calls.append(["prefill", slots, lens])
            r = 0
            with self.own():
                for b, (s, n) in enumerate(zip(slots, lens)):
                    toks = [int(t) for t in emb[r:r + n, 0].float().tolist()]
                    assert 0 <= s < self.n_slots and pos[0, r:r + n].tolist() == list(range(n))
                    self.cache[s] = toks
                    hid_out[r:r + n] = emb[r:r + n]
                    logits_out[b] = toy_logits(toks)
                    r += n

        def gather_slots(self, slots, copy_src, lengths):
            self.mark()
            with self.own():
                src = copy_src.tolist()
            slots, lengths = [int(s) for s in slots], [int(v) for v in lengths]
            assert len(src) == len(slots) == len(lengths) and len(set(slots)) == len(slots)
            self.calls.append(["gather", src])
            dst_rows = {j for j, c in enumerate(src) if c >= 0}
            assert not dst_rows & {c for c in src if c >= 0}, "a row is written and read by one gather"
            for j in sorted(dst_rows):
                held = self.cache[slots[src[j]]]
                assert len(held) == lengths[j], "the length the host names is not what the source holds"
                self.cache[slots[j]] = list(held)

        def _decode_slots(self, n, slots_np, tok_dev, pos_dev, cache_np, hid_out, logits_out):
            self.mark()
            with self.own():
                slots, toks, pos = [int(s) for s in slots_np[:n]], tok_dev[:n].tolist(), pos_dev.tolist()
            assert len(set(slots)) == n and all(s in self.cache for s in slots), "a decode row names a slot that holds nothing"
            self.calls.append(["decode", slots, toks])
            step = len(self.held)
            for i, s in enumerate(slots):
                assert int(cache_np[i]) == len(self.cache[s]) < self.slot_len, "cache length out of step with the slot's contents"
                assert [p[i] for p in pos] == [len(self.cache[s])] * 3
                assert 0 <= toks[i] < V, "a token outside the vocabulary is fed"
                hid_out[i].zero_()
                hid_out[i, 0], hid_out[i, 1], hid_out[i, 2], hid_out[i, 3] = float(toks[i]), float(s), float(step), float(len(self.cache[s]))
                self.cache[s].append(toks[i])
                logits_out[i] = toy_logits(self.cache[s])
            self.held.append({s: list(self.cache[s]) for s in slots})

    e = Fake()

    def logprobs_rows(logits, ids, n_top, top_cap):
        e.mark()
        n = logits.shape[0]
        with e.own():
            want = n_top.tolist()
            e.calls.append(["logprobs_rows", want, int(top_cap)])
            lp = torch.log_softmax(logits.float(), dim=1)
            tid, tlp = torch.full((n, top_cap), -1, dtype=torch.int32), torch.full((n, top_cap), float("-inf"))
            for i in range(n):
                if want[i] >= 0:
                    row = lp[i].tolist()
                    order = sorted(range(V), key=lambda t: (-row[t], t))[:min(want[i], top_cap)]
                    tid[i, :len(order)] = torch.tensor(order, dtype=torch.int32)
                    tlp[i, :len(order)] = lp[i][order]
        return torch.full((n,), float("-inf")), torch.zeros(n, dtype=torch.int32), tid, tlp

    def beam_select(top_ids, top_lp, cum_in, rank_in, W, n_in, eos, token, cum_out, rank_out, copy_src, parent, fin_flag, fin_cum):
        e.mark()
        with e.own():
            ref = select_ref(top_ids.numpy(), top_lp.numpy(), cum_in.numpy(), rank_in.numpy(), W, n_in, eos)
            e.calls.append(["beam_select", int(W), int(n_in), int(eos), int(ref["fin_flag"].sum())])      # (.., the finishers of the step)
            for t, k in zip((token, cum_out, rank_out, copy_src, parent, fin_flag, fin_cum), OUT_KEYS):
                t.copy_(torch.from_numpy(ref[k]))

    return e, Q, SimpleNamespace(logprobs_rows=logprobs_rows, beam_select=beam_select)


def patch(monkeypatch, e, Q, ops):
    """The stand-in's ops in place of torch.ops.thinkdiff_hip, and a counter on every way a tensor reaches the host."""
    monkeypatch.setattr(Q, "_OPS", ops)
    for name in DOWNLOADS:
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **kw):
            e.count()
            with e.own():      # (tolist() may itself go through item())
                return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
