"""Automatic prefix caching for the Qwen2-VL decode engine ([ext] vLLM V1 `enable_prefix_caching`): the host side.

A request whose prompt begins with rows some cache slot already holds does not compute them again.  The engine's KV cache is n_slots whole sequences, not
a pool of blocks, so a hit is served from a DONOR slot: its rows [0, m) are taken over in place (the donor is retained and nobody else wants it in this
pass) or copied to the request's slot (one td_qwen2_fork_slot launch per donor and match length), and the packed prefill behind cached prefixes
(td_qwen2_prefill_packed_prefix_slots) computes the rest.  Deviations from vLLM, stated: only PROMPT rows are cached, generated rows are not; blocks are
never shared in place between live sequences; there is no `cache_salt`.

Keys.  Blocks of 16 tokens (vLLM's block size).  The hash of block j chains the parent block's hash, the block's token ids, the block's
position_ids[:, 16j:16j+16] -- the cached keys are rotated by them, so equal tokens at other M-RoPE positions are other keys -- and, for a request with
inputs_embeds, an identity of those rows: the request's "mm_hash" (str or bytes, vLLM's multimodal hash) with the row range, or, without one, the rows'
bytes read back to the host.  hashlib.blake2b, never Python's per-process hash().

Entries.  slot -> (block hashes of its prompt, the prompt's hidden rows [n, D] on the device, last-use tick, live or retained).  A sequence that
finishes leaves its slot retained; retained slots are handed out only after the free ones are gone, least recently used first.

This module knows no engine: PrefixCache.plan_pass decides, Qwen2VLTextEngine carries it out (tests/test_prefix_cache_cpu.py runs it on a stand-in).
"""
import hashlib
import struct
from typing import List, Optional, Sequence

import numpy as np
import torch

BLOCK = 16
_ROOT = b"thinkdiff-prefix-cache/16"

STAT_KEYS = ("queries", "hits", "passes", "copies", "copied_rows", "in_place", "deferred", "evictions", "hidden_bytes")


def _as_bytes(x) -> bytes:
    return x if isinstance(x, (bytes, bytearray)) else str(x).encode("utf-8")


def block_hashes(token_ids: Sequence[int], position_ids, inputs_embeds=None, mm_hash=None, adapter=None) -> List[bytes]:
    """The chained hashes of the FULL blocks of a prompt (len(token_ids) // 16 of them).  position_ids: [3, n] ints.  inputs_embeds: the request's
    embedding rows [n, D] or None; mm_hash: their identity (str / bytes) -- without one the rows' bytes are read back to the host and hashed.
    adapter: the identity of the request's LoRA adapter (an int id, str or bytes; vLLM hashes the LoRA id into a block's extra keys): it salts the root, so
    the same prompt under two adapters shares no block -- the cached keys and values came through the adapter's k_proj / v_proj.  None: the hashes of the
    base model, bit for bit what they were before adapters existed."""
    n = len(token_ids)
    nb = n // BLOCK
    if nb == 0:
        return []
    tok = np.ascontiguousarray(np.asarray(list(token_ids[:nb * BLOCK]), dtype=np.int32))
    pos = position_ids.detach().to("cpu", torch.int32).numpy() if torch.is_tensor(position_ids) else np.asarray(position_ids, dtype=np.int32)
    if pos.shape != (3, n):
        raise ValueError(f"prefix cache: position_ids of shape {tuple(pos.shape)} for a prompt of {n} tokens (expected (3, {n}))")
    rows = ident = None
    if inputs_embeds is not None:
        if mm_hash is not None:
            ident = b"mm:" + _as_bytes(mm_hash)
        else:      # one read-back of the rows the full blocks cover
            rows = inputs_embeds[:nb * BLOCK].detach().contiguous().view(torch.int16 if inputs_embeds.element_size() == 2 else torch.int32).cpu().numpy()
    out, parent = [], hashlib.blake2b(_ROOT if adapter is None else _ROOT + b"/lora:" + _as_bytes(adapter), digest_size=16).digest()
    for j in range(nb):
        a, b = j * BLOCK, (j + 1) * BLOCK
        h = hashlib.blake2b(parent, digest_size=16)
        h.update(tok[a:b].tobytes())
        h.update(np.ascontiguousarray(pos[:, a:b]).tobytes())
        if ident is not None:
            h.update(ident + struct.pack("<qq", a, b))
        elif rows is not None:
            h.update(b"rows:" + rows[a:b].tobytes())
        parent = h.digest()
        out.append(parent)
    return out


def image_digest(images) -> bytes:
    """An "mm_hash" from the image bytes on the host (PIL images, arrays or tensors; one or a list): what the model classes put into an image request while
    the feature is on, so that it costs no device read-back."""
    h = hashlib.blake2b(digest_size=16)
    for im in (images if isinstance(images, (list, tuple)) else [images]):
        if hasattr(im, "tobytes") and hasattr(im, "mode") and hasattr(im, "size"):      # PIL
            h.update(f"pil:{im.mode}:{im.size[0]}x{im.size[1]}:".encode())
            h.update(im.tobytes())
        else:
            a = im.detach().cpu().contiguous().numpy() if torch.is_tensor(im) else np.ascontiguousarray(np.asarray(im))
            h.update(f"arr:{a.dtype}:{a.shape}:".encode())
            h.update(a.tobytes())
    return h.digest()


class _Entry:
    __slots__ = ("hashes", "hidden", "tick", "live")

    def __init__(self, hashes, hidden, tick):
        self.hashes, self.hidden, self.tick, self.live = hashes, hidden, tick, True


class Placement:
    """One request of a pass: its cache slot, the donor of its first m rows (None: a miss, m = 0) and whether the donor's slot was taken over in place."""
    __slots__ = ("slot", "donor", "m", "in_place")

    def __init__(self, slot, donor, m, in_place):
        self.slot, self.donor, self.m, self.in_place = slot, donor, m, in_place


class PrefixCache:
    def __init__(self, n_slots: int):
        self.stats = {k: 0 for k in STAT_KEYS if k != "hidden_bytes"}
        self.resize(n_slots)

    # ---- slots ------------------------------------------------------------------------------------------------------------------------------------
    def resize(self, n_slots: int):
        """Forget everything; n_slots free slots (the lowest is handed out first)."""
        self.n_slots = int(n_slots)
        self.entries = {}               # slot -> _Entry
        self.index = {}                 # block hash -> slots whose prompt holds that block (the chain makes a hash name its whole prefix)
        self.taken = set()              # slots handed out that hold no entry (children of n / best_of, beams, a pass in flight)
        self.free = list(range(self.n_slots - 1, -1, -1))
        self.tick = 0

    def clear(self):
        self.resize(self.n_slots)

    def _unindex(self, slot):
        e = self.entries.pop(slot, None)
        if e is not None:
            for h in e.hashes:
                s = self.index.get(h)
                if s is not None:
                    s.discard(slot)
                    if not s:
                        del self.index[h]
        return e

    def _give_back(self, slot):
        if slot not in self.free:
            self.free.append(slot)
            self.free.sort(reverse=True)

    def retained(self):
        return [s for s, e in self.entries.items() if not e.live]

    def available(self, protect=()) -> int:
        """Slots take() can hand out while `protect` must stay."""
        return len(self.free) + sum(1 for s in self.retained() if s not in protect)

    def take(self, k: int, protect=()) -> Optional[List[int]]:
        """k slots for new sequences: free ones first, then retained ones, least recently used first, never one of `protect`.  None (and nothing
        changed) when there are not that many."""
        if k > self.available(protect):
            return None
        out = []
        lru = sorted((s for s in self.retained() if s not in protect), key=lambda s: (self.entries[s].tick, s))
        for _ in range(k):
            if self.free:
                s = self.free.pop()
            else:
                s = lru.pop(0)
                self._unindex(s)
                self.stats["evictions"] += 1
            self.taken.add(s)
            out.append(s)
        return out

    def insert(self, slot: int, hashes: List[bytes], hidden):
        """`slot` now holds a live sequence whose prompt has these block hashes and hidden rows."""
        self._unindex(slot)
        self.taken.discard(slot)
        if slot in self.free:
            self.free.remove(slot)
        self.tick += 1
        self.entries[slot] = _Entry(list(hashes), hidden, self.tick)
        for h in hashes:
            self.index.setdefault(h, set()).add(slot)

    def release(self, slot: int):
        """The sequence in `slot` finished: its prompt stays, retained; a slot without an entry is free again."""
        e = self.entries.get(slot)
        if e is not None:
            self.tick += 1
            e.live, e.tick = False, self.tick
        elif slot in self.taken:
            self.taken.discard(slot)
            self._give_back(slot)

    def release_all(self):
        for s in [s for s, e in self.entries.items() if e.live] + list(self.taken):
            self.release(s)

    def drop(self, slot: int):
        """Somebody wrote `slot` behind the cache's back (or its rows are stale): forget what it held."""
        if 0 <= slot < self.n_slots:
            self._unindex(slot)
            self.taken.discard(slot)
            self._give_back(slot)

    # ---- lookup and placement -------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def cap_blocks(n_tokens: int) -> int:
        """Blocks a match may cover: at least one row is always computed, so the last token's logits exist."""
        return (n_tokens - 1) // BLOCK

    def lookup(self, hashes: List[bytes], n_tokens: int):
        """-> (donor slot or None, m): the longest chain of full blocks a live or retained slot holds, capped at ((n - 1) // 16) * 16 rows.  Among the
        holders a retained slot is preferred (it may be taken over without a copy), then the most recently used."""
        nb = 0
        cap = min(self.cap_blocks(n_tokens), len(hashes))
        while nb < cap and hashes[nb] in self.index:
            nb += 1
        if nb == 0:
            return None, 0
        donor = min(self.index[hashes[nb - 1]], key=lambda s: (self.entries[s].live, -self.entries[s].tick, s))
        return donor, nb * BLOCK

    def plan_pass(self, items, max_requests: int, row_budget: int, stage_budget: Optional[int] = None) -> List[Placement]:
        """One prefill pass over the head of `items` = [(block hashes, prompt length)] in arrival order -> a Placement for each of the first t of them.

        A request whose match with an EARLIER request of this pass is longer than its match with the cache is deferred: the pass ends in front of it, and in
        the following pass that earlier request is its donor (eight questions about one image: one leader, then seven followers).  Nobody overtakes it.  The
        pass also ends where the new rows exceed row_budget, the staged rows (prefix + new, the e4m3 cache) stage_budget, or the requests max_requests.
        A retained donor with exactly one taker is taken over in place; every other taker gets a slot of its own -- free first, then the least recently used
        retained one, never a donor of this pass -- and the pass is cut short where those run out.  Updates the statistics; the caller enqueues
        copies() in front of the prefill and reports the result with insert()."""
        chosen, seen, rows, staged = [], set(), 0, 0
        for hashes, n in items:
            if len(chosen) >= max_requests:
                break
            donor, m = self.lookup(hashes, n)
            cap, mp = min(self.cap_blocks(n), len(hashes)), 0
            while mp < cap and hashes[mp] in seen:
                mp += 1
            if mp * BLOCK > m:
                self.stats["deferred"] += 1
                break
            if chosen and (rows + n - m > row_budget or (stage_budget is not None and staged + n > stage_budget)):
                break
            chosen.append((donor, m, n))
            seen.update(hashes)
            rows, staged = rows + n - m, staged + n
        while chosen:
            takers = {}
            for donor, m, _ in chosen:
                if donor is not None:
                    takers[donor] = takers.get(donor, 0) + 1
            in_place = {d for d, c in takers.items() if c == 1 and not self.entries[d].live}
            protect = set(takers)
            if len(chosen) - len(in_place) <= self.available(protect):
                break
            chosen.pop()
        out = []
        for donor, m, n in chosen:
            if donor is not None and donor in in_place:
                self.entries[donor].live = True
                slot = donor
                self.stats["in_place"] += 1
            else:
                slot = self.take(1, protect)[0]
            out.append(Placement(slot, donor, m, donor is not None and donor in in_place))
            self.stats["queries"] += n
            self.stats["hits"] += m
        if out:
            self.stats["passes"] += 1
        return out

    def copies(self, plan: List[Placement]):
        """The copies of a pass: [(donor, m, destination slots)], one per donor and match length.  No destination is a donor of the pass."""
        groups = {}
        for p in plan:
            if p.donor is not None and not p.in_place:
                groups.setdefault((p.donor, p.m), []).append(p.slot)
        out = [(d, m, dsts) for (d, m), dsts in groups.items()]
        donors = {p.donor for p in plan if p.donor is not None}
        assert not any(s in donors for _, _, dsts in out for s in dsts), "prefix cache: a donor of the pass is also a copy destination"
        self.stats["copies"] += len(out)
        self.stats["copied_rows"] += sum(m * len(dsts) for _, m, dsts in out)
        return out

    def hidden_of(self, slot: int):
        return self.entries[slot].hidden

    def get_stats(self) -> dict:
        out = dict(self.stats)
        out["hidden_bytes"] = sum(int(e.hidden.numel()) * int(e.hidden.element_size()) for e in self.entries.values() if e.hidden is not None)
        return out


def zero_stats() -> dict:
    return {k: 0 for k in STAT_KEYS}
