"""The stand-in engine of tests/parallel_sampling_common.py, extended for automatic prefix caching (tests/test_prefix_cache_cpu.py): the prefill behind
cached prefixes and the copy of a hit are replaced by the toy model, which CHECKS the caller on every call.

The stand-in keeps, per cache slot, the token AND position list of the rows it holds -- all of them, retained slots included: a slot keeps its rows until
somebody writes it, exactly like the device cache.  _prefill_packed_prefix_slots asserts that rows [0, prefix) of the named slot hold exactly the request's
first `prefix` tokens at the request's first `prefix` positions (the stand-in learns the whole prompt from `expect`, which the test fills: the engine call
carries the new rows only), that the pass fits the workspace, and _prefix_copy that no destination of a copy is a donor of the same pass.  Any false hit,
stale donor or eviction race fails here.
"""
import torch

import parallel_sampling_common as PS

V, D = PS.V, PS.D


def fake_engine(n_slots, slot_len=256, prefill_rows=512, caching=True):
    base, Q, ops = PS.fake_engine(n_slots, slot_len, prefill_rows)

    class Fake(type(base)):
        packed_prefill = True

        def __init__(self):
            super().__init__()
            self.rows = {}           # slot -> [(token, position)] of every row the slot holds, live or retained
            self.pass_donors = set()
            self.pass_dsts = set()
            self.prefix_calls = []   # (slots, new lens, prefix lens) per pass
            self.copies_log = []     # (src, dsts, length)
            self.computed_rows = 0
            self.set_prefix_caching(caching)

        # (the parent's writers: keep `rows` in step with what they hold)
        def _hold(self, slot, toks, pos=None):
            super()._hold(slot, toks)
            self.rows[slot] = list(zip(toks, range(len(toks)) if pos is None else pos))

        def _prefill_packed_slots(self, k, slots_c, emb, pos, lens_c, hid_out, logits_out):
            super()._prefill_packed_slots(k, slots_c, emb, pos, lens_c, hid_out, logits_out)
            self.computed_rows += sum(lens_c)

        def forward(self, position_ids, token_ids=None, inputs_embeds=None, pos0=0, want_hidden=True, want_logits=False, slot=0):
            out = super().forward(position_ids, token_ids, inputs_embeds, pos0, want_hidden, want_logits, slot)
            if not want_logits:
                self.rows.pop(slot, None)      # (a prompt-only forward: the slot holds nothing anybody may rely on)
            self.computed_rows += position_ids.shape[1]
            return out

        def _step(self, slots, toks, cache_pos, pos_rows, hid_out, logits_out):
            super()._step(slots, toks, cache_pos, pos_rows, hid_out, logits_out)
            for i, s in enumerate(slots):
                self.rows[s] = self.rows[s][:int(cache_pos[i])] + [(int(toks[i]), int(pos_rows[0][i]))]

        def _fork_slots(self, src, dst_slots, length):
            super()._fork_slots(src, dst_slots, length)
            for d in dst_slots:
                self.rows[int(d)] = list(self.rows[int(src)][:int(length)])

        # ---- the two calls prefix caching adds ----
        def _prefix_copy(self, src, dst_slots, length):
            src, dst, length = int(src), [int(d) for d in dst_slots], int(length)
            assert dst and len(set(dst)) == len(dst) and src not in dst
            assert len(self.rows.get(src, [])) >= length > 0, f"copy of {length} rows from slot {src}, which holds {len(self.rows.get(src, []))}"
            assert length % 16 == 0
            self.pass_donors.add(src)
            self.pass_dsts.update(dst)
            assert not (self.pass_donors & self.pass_dsts), "a donor of the pass is also a copy destination"
            self.copies_log.append((src, dst, length))
            self.calls.append(["prefix_copy", src, dst, length])
            for d in dst:
                assert 0 <= d < self.n_slots      # (a copy into a slot whose sequence still decodes shows at that sequence's next step: its cache length is out of step)
                self.rows[d] = list(self.rows[src][:length])

        def _prefill_packed_prefix_slots(self, k, slots_c, emb, pos, lens_c, prefix_c, hid_out, logits_out):
            slots, lens, prefixes = list(slots_c), list(lens_c), list(prefix_c)
            assert len(set(slots)) == k and sum(lens) == emb.shape[0] <= self.prefill_rows and pos.shape == (3, sum(lens)), "the pass does not fit"
            self.prefix_calls.append((slots, lens, prefixes))
            self.calls.append(["prefix_prefill", slots, lens, prefixes])
            r = 0
            for b, (s, n, p) in enumerate(zip(slots, lens, prefixes)):
                assert n >= 1 and p >= 0 and p % 16 == 0 and p + n <= self.slot_len and 0 <= s < self.n_slots
                new = [int(t) for t in emb[r:r + n, 0].float().tolist()]
                new_pos = pos[0, r:r + n].tolist()
                full = self.expect.pop(0)      # the whole prompt this sequence stands for, in call order
                assert full["tokens"][p:] == new and full["pos"][p:] == new_pos, "the new rows are not the prompt's rows behind the prefix"
                held = self.rows.get(s, [])
                assert len(held) >= p and held[:p] == list(zip(full["tokens"][:p], full["pos"][:p])), \
                    f"slot {s} does not hold the first {p} rows of the prompt: a false hit, a stale donor or an evicted one"
                self._hold(s, full["tokens"], full["pos"])
                self.prefilled.append(full["tokens"])
                hid_out[r:r + n] = emb[r:r + n]
                self._logits_for(new[-1], logits_out[b])
                self.computed_rows += n
                r += n
            self.pass_donors, self.pass_dsts = set(), set()

    e = Fake()
    e.expect = []
    return e, Q, ops


def expect_prompts(e, requests, poss=None):
    """Tell the stand-in which whole prompts the coming prefix prefills stand for, in the order the engine will place them (arrival order)."""
    for i, q in enumerate(requests):
        n = len(q["prompt_token_ids"])
        p = q.get("position_ids")
        e.expect.append({"tokens": [int(t) for t in q["prompt_token_ids"]], "pos": list(range(n)) if p is None else [int(x) for x in p[0].tolist()]})


def shared_prompts(n, shared_blocks, seed=3, tail_lo=1, tail_hi=20, prefix_seed=None):
    """n requests that share shared_blocks x 16 tokens and differ in their tails (the first tail token differs between any two)."""
    g = torch.Generator().manual_seed(seed)
    gp = torch.Generator().manual_seed(seed if prefix_seed is None else prefix_seed)
    head = torch.randint(0, V, (16 * shared_blocks,), generator=gp).tolist()
    out = []
    for i in range(n):
        tail = torch.randint(0, V, (tail_lo + int(torch.randint(0, tail_hi - tail_lo + 1, (1,), generator=g)),), generator=g).tolist()
        tail[0] = (7 + i) % V
        out.append({"prompt_token_ids": head + tail})
    return out
