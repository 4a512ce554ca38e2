"""The stand-in engine of tests/parallel_sampling_common.py with a verify call, for the host logic of speculative decoding
(tests/test_spec_decode_cpu.py).

  verify    _verify_slots: live row i feeds n_new[i] tokens at cache rows cache_pos[i] ..; the "model" is the stand-in's deterministic token function,
            so row (i, j) has one-hot logits at next_token(fed token) and echoes (token, slot) in its hidden row.  The call CHECKS what the loop may
            not do -- a fed row past the slot's capacity, positions out of step, more than 8 rows per sequence or 256 per step -- and logs
            ["verify", slots, n_new, fed tokens].  Rows of rejected tokens stay in the slot's `written` list and are overwritten, as on the device;
            the slot's `cache` holds only what the caller has advanced over, which the next call's cache_pos must match.
  accept    spec_accept: the rule of td_spec_accept as a numpy loop.

Draft sources: OracleDraft guesses what the token function will produce (every guess is accepted at temperature 0), WrongDraft never does.
"""
import numpy as np
import torch

import parallel_sampling_common as P

V, D = P.V, P.D
next_token = P.next_token


class OracleDraft:
    """Knows the stand-in model: guess j is the token function applied j times to the last token."""

    def propose(self, token_ids, k):
        out, t = [], int(token_ids[-1])
        for _ in range(int(k)):
            t = next_token(t)
            out.append(t)
        return np.array(out, dtype=np.int32)


class WrongDraft:
    def propose(self, token_ids, k):
        return np.array([(next_token(int(token_ids[-1])) + 1) % V] * int(k), dtype=np.int32)


def accept_ref(sampled, fed, row0, rows):
    B = len(row0)
    n_emit, emit = np.zeros(B, dtype=np.int32), np.full((B, 8), -1, dtype=np.int32)
    for b in range(B):
        a = 0
        while a < rows[b] - 1 and fed[row0[b] + a + 1] == sampled[row0[b] + a]:
            a += 1
        n_emit[b] = a + 1
        emit[b, :a + 1] = sampled[row0[b]:row0[b] + a + 1]
    return n_emit, emit


def fake_engine(n_slots, slot_len=64, prefill_rows=96):
    e, Q, ops = P.fake_engine(n_slots, slot_len, prefill_rows)
    e.verify_rows = []       # (slot, cache_pos, n_new) of every sequence of every verify call

    def _verify_slots(n, slots_np, n_new_np, tok_dev, pos_dev, cache_np, hid_out, logits_out):
        slots, n_new, toks = [int(x) for x in slots_np[:n]], [int(x) for x in n_new_np[:n]], tok_dev.tolist()
        for s in e.last_live - set(slots):
            e.cache.pop(s, None)
        assert len(set(slots)) == n and all(s in e.cache for s in slots), "a verify row names a slot that was neither prefilled nor forked, or a repeated one"
        e.last_live = set(slots)
        R = sum(n_new)
        assert R <= 256 and len(toks) == R and tuple(pos_dev.shape) == (3, R) and hid_out.shape[0] == R and logits_out.shape[0] == R
        e.max_rows = max(e.max_rows, R)
        e.calls.append(["verify", slots, n_new, [int(t) for t in toks]])
        r = 0
        for i, s in enumerate(slots):
            have = len(e.cache[s])
            assert 1 <= n_new[i] <= 8, "a sequence feeds 1..8 rows"
            assert int(cache_np[i]) == have, "cache length out of step with what the caller advanced over"
            assert have + n_new[i] <= e.slot_len, "a fed row past the slot's capacity"
            e.verify_rows.append((s, have, n_new[i]))
            for j in range(n_new[i]):
                assert [int(p[r]) for p in pos_dev] == [have + j] * 3
                t = int(toks[r])
                hid_out[r].zero_()
                hid_out[r, 0], hid_out[r, 1] = float(t), float(s)
                e._logits_for(t, logits_out[r])
                r += 1
            e.pending = getattr(e, "pending", {})
            e.pending[s] = toks[r - n_new[i]:r]
            e.fresh[s] = False

    def _step_after_verify(orig):
        def step(slots, toks, cache_pos, pos_rows, hid_out, logits_out):
            _settle(slots, cache_pos)
            return orig(slots, toks, cache_pos, pos_rows, hid_out, logits_out)
        return step

    def _settle(slots, cache_pos):
        """The caller advanced slot s by cache_pos - len(cache): those tokens of the last verify were kept, the rest are stale rows."""
        pend = getattr(e, "pending", {})
        for i, s in enumerate(slots):
            if s in pend and s in e.cache:
                k = int(cache_pos[i]) - len(e.cache[s])
                assert 0 <= k <= len(pend[s]), "the caller advanced by more rows than the last verify fed"
                e.cache[s].extend(pend.pop(s)[:k])

    def verify_settled(n, slots_np, n_new_np, tok_dev, pos_dev, cache_np, hid_out, logits_out):
        _settle([int(x) for x in slots_np[:n]], cache_np)
        return _verify_slots(n, slots_np, n_new_np, tok_dev, pos_dev, cache_np, hid_out, logits_out)

    e._verify_slots = verify_settled
    e._step = _step_after_verify(e._step)

    def spec_accept(sampled, fed, seq_row0, seq_rows):
        e.calls.append(["spec_accept", seq_rows.tolist()])
        n_emit, emit = accept_ref(sampled.numpy(), fed.numpy(), seq_row0.numpy(), seq_rows.numpy())
        return torch.from_numpy(n_emit), torch.from_numpy(emit)

    ops.spec_accept = spec_accept
    return e, Q, ops


patch = P.patch
prompts = P.prompts
