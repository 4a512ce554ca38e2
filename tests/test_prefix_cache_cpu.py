"""Automatic prefix caching, host side (thinkdiff/models/prefix_cache.py and its place in Qwen2VLTextEngine's entries), against the stand-in engine of
tests/prefix_cache_common.py, which asserts on every prefill that the slot holds exactly the prefix the caller claims.  No GPU."""
import hashlib
import random
import re

import numpy as np
import pytest
import torch

import parallel_sampling_common as PS
import prefix_cache_common as PC

V = PC.V


@pytest.fixture
def eng(monkeypatch):
    def make(n_slots, caching=True, **kw):
        e, Q, ops = PC.fake_engine(n_slots, caching=caching, **kw)
        PS.patch(monkeypatch, Q, ops)
        return e, Q
    return make


def _sp(Q, k=3, **kw):
    return Q.SamplingParams(temperature=0.0, max_tokens=k, min_tokens=k, **kw)


def _batch(e, Q, reqs, k=3, **kw):
    PC.expect_prompts(e, reqs)
    return e.generate_batch(reqs, _sp(Q, k), **kw)


def _delta(e, before):
    now = e.prefix_cache_stats()
    return {k: now[k] - before[k] for k in now}


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------------
def test_hash_chain():
    from thinkdiff.models import prefix_cache as M
    toks = list(range(40))
    pos = torch.arange(40, dtype=torch.int32)[None].expand(3, 40).contiguous()
    h = M.block_hashes(toks, pos)
    assert len(h) == 2 and all(isinstance(x, bytes) and len(x) == 16 for x in h) and h[0] != h[1]
    assert M.block_hashes(toks, pos) == h and M.block_hashes(toks[:39], pos[:, :39]) == h, "the hashes of the full blocks depend on those blocks only"
    # the chain, restated: blake2b over (parent, token bytes, position bytes)
    parent = hashlib.blake2b(M._ROOT, digest_size=16).digest()
    want = []
    for j in range(2):
        x = hashlib.blake2b(parent, digest_size=16)
        x.update(np.arange(16 * j, 16 * j + 16, dtype=np.int32).tobytes())
        x.update(np.ascontiguousarray(pos.numpy()[:, 16 * j:16 * j + 16]).tobytes())
        parent = x.digest()
        want.append(parent)
    assert h == want
    # a change in block 0 changes every later hash; a change in block 1 leaves block 0
    t2 = list(toks); t2[3] += 1
    assert M.block_hashes(t2, pos)[0] != h[0] and M.block_hashes(t2, pos)[1] != h[1]
    t3 = list(toks); t3[20] += 1
    assert M.block_hashes(t3, pos)[0] == h[0] and M.block_hashes(t3, pos)[1] != h[1]
    # position ids are part of the key (the cached keys are rotated by them): one stream shifted in the second block
    p2 = pos.clone(); p2[1, 16:] += 5
    assert M.block_hashes(toks, p2)[0] == h[0] and M.block_hashes(toks, p2)[1] != h[1]
    # inputs_embeds: identified by mm_hash + the row range, or by the rows' bytes
    g = torch.Generator().manual_seed(0)
    e1, e2 = torch.randn(40, 8, generator=g).bfloat16(), torch.randn(40, 8, generator=g).bfloat16()
    assert M.block_hashes(toks, pos, e1) != h and M.block_hashes(toks, pos, e1) == M.block_hashes(toks, pos, e1.clone())
    assert M.block_hashes(toks, pos, e1)[0] != M.block_hashes(toks, pos, e2)[0], "equal placeholder ids, other embeddings: other keys"
    e3 = e1.clone(); e3[20, 0] += 1
    assert M.block_hashes(toks, pos, e3)[0] == M.block_hashes(toks, pos, e1)[0] and M.block_hashes(toks, pos, e3)[1] != M.block_hashes(toks, pos, e1)[1]
    a = M.block_hashes(toks, pos, e1, mm_hash="img-a")
    assert a == M.block_hashes(toks, pos, e2, mm_hash=b"img-a"), "mm_hash IS the identity: the rows are not read"
    assert a[0] != M.block_hashes(toks, pos, e1, mm_hash="img-b")[0] and a != M.block_hashes(toks, pos, e1)
    with pytest.raises(ValueError, match="position_ids of shape"):
        M.block_hashes(toks, pos[:, :30])
    assert M.image_digest([np.zeros((4, 4, 3), np.uint8)]) != M.image_digest([np.ones((4, 4, 3), np.uint8)])


def test_python_hash_is_not_used():
    from thinkdiff.models import prefix_cache as M
    src = open(M.__file__).read()

    assert "hashlib.blake2b" in src
    assert not re.search(r"(?<![\w.])hash\(", src.replace("hash()", "")), "Python's hash() is salted per process: it must not key the cache"
    # and the keys do not depend on PYTHONHASHSEED: the digest of a fixed block is a constant
    pos = torch.arange(16, dtype=torch.int32)[None].expand(3, 16).contiguous()
    assert M.block_hashes(list(range(16)), pos)[0].hex() == M.block_hashes(tuple(range(16)), pos.numpy())[0].hex()


# ---- lookup, placement -------------------------------------------------------------------------------------------------------------------------------
def test_cap_leaves_one_row_to_compute(eng):
    e, Q = eng(4)
    for n, want in ((32, 16), (33, 32), (16, 0), (17, 16), (48, 32)):
        e.reset_prefix_cache()
        req = [{"prompt_token_ids": [(5 * i + n) % V for i in range(n)]}]
        _batch(e, Q, req)
        s0 = e.prefix_cache_stats()
        r = _batch(e, Q, req)      # verbatim
        d = _delta(e, s0)
        assert d["queries"] == n and d["hits"] == want == ((n - 1) // 16) * 16, (n, d)
        assert e.prefix_calls[-1][1:] == ([n - want], [want])
        assert r[0]["prompt_hidden_states"].shape[0] == n


def test_in_place_take_over_against_copy(eng):
    e, Q = eng(6)
    a, b, c, d = PC.shared_prompts(4, 3)
    _batch(e, Q, [a])
    slot_a = e.prefix_calls[-1][0][0]
    s0 = e.prefix_cache_stats()
    _batch(e, Q, [b])      # one taker of a retained donor: its slot, no copy
    dl = _delta(e, s0)
    assert dl["in_place"] == 1 and dl["copies"] == 0 and dl["hits"] == 48 and e.prefix_calls[-1] == ([slot_a], [len(b["prompt_token_ids"]) - 48], [48])
    assert not e.copies_log
    s0 = e.prefix_cache_stats()
    _batch(e, Q, [c, d])   # two takers of one retained donor: both copy, ONE launch, and the donor keeps its prompt
    dl = _delta(e, s0)
    assert dl["in_place"] == 0 and dl["copies"] == 1 and dl["copied_rows"] == 96 and dl["hits"] == 96 and dl["passes"] == 1
    src, dsts, m = e.copies_log[-1]
    assert src == slot_a and m == 48 and len(dsts) == 2 and slot_a not in dsts and e.prefix_calls[-1][0] == dsts
    s0 = e.prefix_cache_stats()
    _batch(e, Q, [b])      # ... which is b's: a verbatim repeat hits up to the cap
    assert _delta(e, s0)["hits"] == ((len(b["prompt_token_ids"]) - 1) // 16) * 16


def test_a_live_donor_is_copied_never_taken(eng):
    e, Q = eng(4)
    a, b = PC.shared_prompts(2, 2)
    PC.expect_prompts(e, [a, b])
    # b arrives while a still decodes (continuous batching, one admission at a time)
    res = e.generate_continuous([a, b], [_sp(Q, 6), _sp(Q, 2)], max_live=2, admit_min=1)
    assert [len(r["token_ids"]) for r in res] == [6, 2]
    assert e.prefix_cache_stats()["deferred"] == 1 and e.prefix_cache_stats()["in_place"] == 0 and len(e.copies_log) == 1


def test_intra_pass_deferral_eight_questions_about_one_image(eng):
    e, Q = eng(8)
    reqs = PC.shared_prompts(8, 6)
    res = _batch(e, Q, reqs)
    st = e.prefix_cache_stats()
    assert [c[2] for c in e.prefix_calls] == [[0], [96] * 7], "one leader, then seven followers behind its 96 rows"
    assert st["hits"] == 7 * 96 and st["queries"] == sum(len(q["prompt_token_ids"]) for q in reqs) and st["deferred"] == 1 and st["passes"] == 2
    assert st["copies"] == 1 and st["copied_rows"] == 7 * 96 and len(e.copies_log[0][1]) == 7
    assert e.computed_rows == st["queries"] - st["hits"]
    off, Q2 = eng(8, caching=False)
    want = off.generate_batch(reqs, _sp(Q2))
    for r, w in zip(res, want):
        assert r["token_ids"] == w["token_ids"] and torch.equal(r["prompt_hidden_states"], w["prompt_hidden_states"]) and torch.equal(r["hidden_states"][:, 0], w["hidden_states"][:, 0])
    assert off.prefix_cache_stats() == {k: 0 for k in st}


def test_lru_eviction_at_four_slots(eng):
    e, Q = eng(4)
    fam = [PC.shared_prompts(2, 2, seed=10 + i, prefix_seed=100 + i) for i in range(6)]
    for i in range(4):
        _batch(e, Q, [fam[i][0]])
    assert e.prefix_cache_stats()["evictions"] == 0
    _batch(e, Q, [fam[0][1]])              # family 0 is used again: now the most recent
    s0 = e.prefix_cache_stats()
    _batch(e, Q, [fam[4][0]])              # a fifth family: the least recently used slot goes, which is family 1's
    assert _delta(e, s0)["evictions"] == 1
    s0 = e.prefix_cache_stats()
    _batch(e, Q, [fam[1][1]])              # family 1 is recomputed (and evicts family 2) ...
    d = _delta(e, s0)
    assert d["hits"] == 0 and d["evictions"] == 1
    s0 = e.prefix_cache_stats()
    _batch(e, Q, [fam[0][0]])              # ... family 0 is still there
    assert _delta(e, s0)["hits"] >= 32


def test_free_slots_go_before_retained_ones(eng):
    e, Q = eng(4)
    a = PC.shared_prompts(1, 2, seed=1)[0]
    b = PC.shared_prompts(1, 2, seed=2, prefix_seed=50)[0]
    _batch(e, Q, [a])
    _batch(e, Q, [b])
    assert e.prefix_calls[0][0] != e.prefix_calls[1][0] and e.prefix_cache_stats()["evictions"] == 0
    s0 = e.prefix_cache_stats()
    _batch(e, Q, [a])
    assert _delta(e, s0)["hits"] == ((len(a["prompt_token_ids"]) - 1) // 16) * 16


# ---- invalidation --------------------------------------------------------------------------------------------------------------------------------------
def _primed(eng):
    e, Q = eng(4)
    a = PC.shared_prompts(1, 3)[0]
    _batch(e, Q, [a])
    slot = e.prefix_calls[-1][0][0]
    return e, Q, a, slot


def _hits_again(e, Q, a):
    s0 = e.prefix_cache_stats()
    _batch(e, Q, [a])
    return _delta(e, s0)["hits"]


@pytest.mark.parametrize("what", ["load_state_dict", "quantize_weights", "set_weight_stream", "set_slots", "reset_prefix_cache", "init_random", "set_prefix_caching"])
def test_whole_cache_invalidations(eng, monkeypatch, what):
    from types import SimpleNamespace
    e, Q, a, slot = _primed(eng)
    assert _hits_again(e, Q, a) == 48
    # the engine methods run on a stand-in handle: only their effect on the cache is looked at
    e._h, e.weight_quantization, e._defer_quantize = None, None, False
    e._L = SimpleNamespace(td_qwen2_quantize_weights=lambda *x: 0, td_qwen2_set_weight_stream=lambda *x: 1, td_qwen2_set_slots=lambda *x: 0,
                           td_qwen2_slot_capacity=lambda *x: e.slot_len, td_qwen2_init_random=lambda *x: 0)
    monkeypatch.setattr(Q._hip, "stream_ptr", lambda: None)
    monkeypatch.setattr(type(e), "param_table", lambda self: {}, raising=False)
    {"load_state_dict": lambda: e.load_state_dict({}, strict=False), "quantize_weights": lambda: e.quantize_weights("fp8"),
     "set_weight_stream": lambda: e.set_weight_stream(True), "set_slots": lambda: e.set_slots(4), "reset_prefix_cache": e.reset_prefix_cache,
     "init_random": lambda: e.init_random(1), "set_prefix_caching": lambda: (e.set_prefix_caching(False), e.set_prefix_caching(True))}[what]()
    assert _hits_again(e, Q, a) == 0, f"{what} left the cache standing"


@pytest.mark.parametrize("what", ["forward", "decode_batch", "verify_batch", "fork_slot", "gather_slots", "move_slot", "prefill_packed"])
def test_low_level_writers_drop_the_slots_they_write(eng, monkeypatch, what):
    from types import SimpleNamespace
    e, Q, a, slot = _primed(eng)
    other = (slot + 1) % 4
    e._h = None
    e._L = SimpleNamespace(**{k: (lambda *x: 0) for k in ("td_qwen2_fork_slot", "td_qwen2_gather_slots", "td_qwen2_move_slot", "td_qwen2_verify_batch_slots",
                                                         "td_qwen2_prefill_packed_prefix_slots")})
    monkeypatch.setattr(Q._hip, "stream_ptr", lambda: None)
    monkeypatch.setattr(Q._hip, "ptr", lambda t: None)
    pos1 = torch.zeros(3, 1, dtype=torch.int32)
    real = Q.Qwen2VLTextEngine

    def run(target):
        e.rows.pop(target, None)      # (what the real call does to the device rows: the stand-in's check would catch a stale hit)
        if what == "forward":
            e._pc_wrote([target])     # the stand-in overrides forward / decode_batch; the real methods call this hook first (asserted below)
        elif what == "decode_batch":
            e._pc_wrote([target])
        elif what == "verify_batch":
            real.verify_batch(e, [1], pos1, [5], [1], slots=[target], want_logits=False)
        elif what == "fork_slot":
            real.fork_slot(e, (target + 2) % 4, [target], 4)
        elif what == "gather_slots":
            real.gather_slots(e, [target], torch.tensor([-1], dtype=torch.int32), [4])
        elif what == "move_slot":
            real.move_slot(e, (target + 2) % 4, target, 4)
        elif what == "prefill_packed":
            e.expect.append({"tokens": [0], "pos": [0]})
            real.prefill_packed(e, [{"position_ids": pos1, "inputs_embeds": torch.zeros(1, PC.D, dtype=torch.bfloat16)}], [target], [0])

    run(other)
    assert _hits_again(e, Q, a) == 48, "a write to another slot must leave the entry"
    run(slot)
    assert _hits_again(e, Q, a) == 0, f"{what} on the slot left its entry standing"
    import inspect
    for name in ("forward", "decode_batch", "verify_batch", "fork_slot", "gather_slots", "move_slot", "prefill_packed"):
        src = inspect.getsource(getattr(real, name))
        assert src.index("_pc_wrote(") < src.index("self._L.td_qwen2_") if "self._L.td_qwen2_" in src else "_pc_wrote(" in src, name


def test_writers_inside_an_entry_keep_the_entries(eng):
    """n = 3: the children's fork goes through fork_slot INSIDE generate_batch; the parent's prompt stays cached, the children's slots are free afterwards."""
    e, Q = eng(6)
    a = PC.shared_prompts(1, 3)[0]
    PC.expect_prompts(e, [a])
    e.generate_batch([a], Q.SamplingParams(temperature=1.0, seed=4, n=3, max_tokens=2, min_tokens=2))
    assert len(e.forks) == 1 and len(e.forks[0][1]) == 2
    assert _hits_again(e, Q, a) == 48 and e.prefix_cache_stats()["in_place"] == 1


# ---- a long random schedule --------------------------------------------------------------------------------------------------------------------------
def test_random_schedule_of_300_requests_over_12_prefixes(eng):
    rnd = random.Random(1234)
    heads = [[rnd.randrange(V) for _ in range(16 * rnd.randint(1, 5))] for _ in range(12)]
    reqs, budgets = [], []
    for i in range(300):
        h = heads[rnd.randrange(12)]
        cut = rnd.choice([len(h), len(h), len(h), max(1, len(h) - rnd.randint(1, 20))])      # mostly the whole head, sometimes a part of it
        tail = [rnd.randrange(V) for _ in range(rnd.randint(0 if cut else 1, 12))]
        reqs.append({"prompt_token_ids": (h[:cut] + tail) or [1]})
        budgets.append(rnd.randint(0, 6))
    forced = [[rnd.randrange(V) for _ in range(b)] for b in budgets]

    def run(caching):
        e, Q = eng(8, caching=caching, slot_len=128, prefill_rows=160)
        PC.expect_prompts(e, [q for q, b in zip(reqs, budgets) if b > 0])
        chunks = [reqs[i:i + 37] for i in range(0, 300, 37)]
        return e, e.generate_continuous(iter(chunks), Q.SamplingParams(max_tokens=8, min_tokens=1), forced_output_ids=forced, max_live=8, admit_min=2)

    on, got = run(True)
    off, want = run(False)
    assert len(got) == 300
    for i, (r, w) in enumerate(zip(got, want)):      # arrival order, and what the uncached run gives
        assert r["token_ids"] == w["token_ids"] == forced[i], i
        assert torch.equal(r["prompt_hidden_states"], w["prompt_hidden_states"]), i
        assert r["prompt_hidden_states"][:, 0].tolist() == [float(t) for t in reqs[i]["prompt_token_ids"]], i
        assert torch.equal(r["hidden_states"][:, 0], w["hidden_states"][:, 0]), i
    st = on.prefix_cache_stats()
    print("random schedule:", st, "rows computed", on.computed_rows, "against", off.computed_rows)
    assert not on.expect, "a prompt the test announced was never prefilled"
    assert st["hits"] > 0 and st["evictions"] > 0 and st["in_place"] > 0 and st["copies"] > 0 and st["deferred"] > 0
    assert on.computed_rows == off.computed_rows - st["hits"], "every hit row is a row not computed"
    assert st["hidden_bytes"] > 0 and st["queries"] == sum(len(q["prompt_token_ids"]) for q, b in zip(reqs, budgets) if b > 0)
