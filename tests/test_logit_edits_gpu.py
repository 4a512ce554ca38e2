"""td_sample_rows_edit_bf16 (bans, allowed ids and logit bias applied in front of the penalties, inside the sampler's launch) on the GPU against the
fp32 / fp64 restatement of tests/logit_edits_common.py under the statistical bars of tests/sampler_rows_common.py, and the engine's logit-edit
path end to end.  Laws are checked as in tests/test_sampler_rows_gpu.py: 16 launches of 4096 rows that differ only in `stream` / `offset`."""
import pytest
import torch

import logit_edits_common as E

pytestmark = pytest.mark.gpu

V = 4096
ROWS, LAUNCHES = 4096, 16


def _row(seed, vocab=V, scale=3.0):
    return (torch.randn(vocab, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16()


def _draws(hip, row, edits, eslot, rows=ROWS, launches=LAUNCHES, sampler=None, seed=1234, **fields):
    """rows x launches draws of one row under edit slot `eslot`: row r of launch o draws from (seed, o, r)."""
    logits = row.cuda()[None].expand(rows, row.numel()).contiguous()
    table = hip.pack_sample_rows([dict(fields, seed=seed, stream=r) for r in range(rows)]).cuda()
    es = torch.full((rows,), eslot, dtype=torch.int32, device="cuda")
    out = [hip.sample_rows_edit(logits, table, torch.full((rows,), o, dtype=torch.int64, device="cuda"), sampler, False, edits, es) for o in range(launches)]
    torch.cuda.synchronize()
    return torch.cat(out).cpu()


def _check_law(hip, row, edits, eslot, z, T, label, min_kept=2, sampler=None, **fields):
    filt = {k: v for k, v in fields.items() if k in ("top_k", "top_p", "min_p")}
    q, edge, p = E.law(z, T, **filt)
    E.check_case(q, p, edge, ROWS * LAUNCHES, min_kept=min_kept, min_p=filt.get("min_p", 0.0))
    d = _draws(hip, row, edits, eslot, sampler=sampler, temperature=T, **fields)
    E.assert_law(d, q, p, edge, label)
    return d, q


@pytest.fixture(scope="module")
def edits(hip):
    e = hip.logit_edits_create(4, V)
    yield e
    e.close()


# ---- 1. no edits: the same bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [152064, 4096])
def test_no_edits_is_sample_rows_bit_for_bit(hip, vocab):
    x = (torch.randn(64, vocab, generator=torch.Generator().manual_seed(vocab + 1)) * 3).bfloat16().cuda()
    e = hip.logit_edits_create(2, vocab)
    e.ban(1, [0, 5, vocab - 1])
    e.set_bias(1, {3: 2.0, vocab - 2: -1.0})
    e.reset_slot(1)                                            # a slot that was used and reset
    s = hip.sampler_create(1, vocab)
    counts = torch.zeros(vocab, dtype=torch.int32)
    counts[torch.randint(0, vocab, (200,), generator=torch.Generator().manual_seed(3))] = 2
    s.set_counts(0, counts)
    cases = [(dict(temperature=0.0), None), (dict(temperature=0.6, top_p=0.9), None), (dict(temperature=0.8, top_k=50, top_p=0.9), None),
             (dict(temperature=0.8, top_k=40, repetition_penalty=1.3, frequency_penalty=0.5, slot=0), s)]
    for fields, state in cases:
        for off in range(2):
            rows = [dict(fields, seed=77, stream=r) for r in range(64)]
            offs = torch.full((64,), off, dtype=torch.int64, device="cuda")
            ref = hip.sample_rows(x, rows, offs, state)
            assert torch.equal(hip.sample_rows_edit(x, rows, offs, state, False, None, None), ref), "e NULL"
            assert torch.equal(hip.sample_rows_edit(x, rows, offs, state, False, e, -1), ref), "every slot -1"
            assert torch.equal(hip.sample_rows_edit(x, rows, offs, state, False, e, [7 if r % 2 else -5 for r in range(64)]), ref), "slots out of range"
            assert torch.equal(hip.sample_rows_edit(x, rows, offs, state, False, e, 1), ref), "a slot that was reset"
    with pytest.raises(hip.ThinkDiffHipError, match="differs from the edit state"):
        hip.sample_rows_edit(torch.zeros(1, 1024, dtype=torch.bfloat16, device="cuda"), [dict()], 0, None, False, e, 0)
    e.close()
    s.close()


# ---- 2. bans ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [dict(), dict(top_k=50, top_p=0.9)])
def test_banned_tokens_are_never_drawn_and_the_law_is_the_masked_one(hip, edits, filt):
    row, T = _row(61), 0.8
    order = torch.argsort(row.float(), descending=True, stable=True)
    banned = sorted(set(order[:10].tolist()) | set(torch.randperm(V, generator=torch.Generator().manual_seed(6))[:1000].tolist()))
    edits.reset_slot(0)
    edits.ban(0, banned + [V + 3, -1])                        # (ids outside the vocabulary are ignored)
    got, _ = edits.read(0)
    mask = torch.zeros(V, dtype=torch.uint8)
    mask[torch.tensor(banned)] = 1
    assert torch.equal(got.cpu(), mask)
    z = E.edited(row, banned)
    d, _ = _check_law(hip, row, edits, 0, z, T, f"bans {filt}", min_kept=5, **filt)
    assert int(torch.bincount(d.long(), minlength=V)[torch.tensor(banned)].sum()) == 0, "a banned id was drawn"
    g = _draws(hip, row, edits, 0, rows=64, launches=1, temperature=0.0)
    assert bool((g == int(z.argmax())).all())


# ---- 3. allow_only ------------------------------------------------------------------------------------------------------------------------
def test_allow_only_at_chunk_and_thread_edges(hip):
    vocab = 8 * 1024 + 4096                                   # (8 x 1024 - 1 is the last token of the first sweep of the 1024 threads)
    ids = [0, 7, 8, 8 * 1024 - 1, vocab - 1]
    row, T = _row(62, vocab=vocab), 1.0
    e = hip.logit_edits_create(1, vocab)
    e.allow_only(0, ids)
    banned = sorted(set(range(vocab)) - set(ids))
    assert e.read(0)[0].cpu().nonzero().flatten().tolist() == banned
    z = E.edited(row, banned)
    q, edge, p = E.law(z, T)
    E.check_case(q, p, edge, ROWS * LAUNCHES, min_kept=2)
    d = _draws(hip, row, e, 0, temperature=T)
    assert set(d.tolist()) <= set(ids)
    E.assert_law(d, q, p, edge, "allow_only, 5 ids")
    d = _draws(hip, row, e, 0, launches=2, temperature=T, top_k=50, top_p=0.95)      # top-k reaching into the banned tokens keeps them out
    assert set(d.tolist()) <= set(ids)
    e.allow_only(0, [])                                        # everything banned: the -inf row rule, id 0, no fault
    assert bool((_draws(hip, row, e, 0, rows=8, launches=1, temperature=T) == 0).all())
    e.close()


# ---- 4. bias ------------------------------------------------------------------------------------------------------------------------------
def test_a_large_bias_lifts_a_tail_token_to_the_top(hip, edits):
    row, T = _row(63), 0.8
    order = torch.argsort(row.float(), descending=True, stable=True)
    tail = int(order[-5])
    bias = {tail: float(row[order[1]]) + 0.5 - float(row[tail]), int(order[0]): -4.0, int(order[3]): 0.3}      # the tail token ends half a unit above the rest
    edits.reset_slot(1)
    edits.set_bias(1, bias)
    got = edits.read(1)[1].cpu()
    assert got.nonzero().flatten().tolist() == sorted(bias) and [float(got[t]) for t in sorted(bias)] == [float(torch.tensor(bias[t])) for t in sorted(bias)]
    z = E.edited(row, (), bias)
    assert int(z.argmax()) == tail
    g = _draws(hip, row, edits, 1, rows=64, launches=1, temperature=0.0)
    assert bool((g == tail).all())
    _check_law(hip, row, edits, 1, z, T, "bias", min_kept=3)
    _check_law(hip, row, edits, 1, z, T, "bias, top_k 20 top_p 0.9", min_kept=3, top_k=20, top_p=0.9)


@pytest.mark.parametrize("filt,kept", [(dict(top_k=2), 2), (dict(top_k=3, top_p=0.9), 3), (dict(top_k=5), 5), (dict(top_p=0.4), 3)])
def test_boundary_among_biased_tokens_of_one_bf16_bucket(hip, edits, filt, kept):
    """Four biased tokens whose fp32 values differ only below bf16 precision (8 - c / 1024, c = 1 .. 4) and an unbiased 7.96875 share one 16-bit key
    bucket, and every boundary falls inside it: the third and fourth radix levels order the edited keys, and the kept count is exact."""
    row = _row(45, scale=1.0)
    ids = [500, 1500, 2500, 3500]
    row[ids] = 8.0
    row[4000] = 7.96875
    bias = {500: -3 / 1024, 1500: -1 / 1024, 2500: -4 / 1024, 3500: -2 / 1024}
    edits.reset_slot(2)
    edits.set_bias(2, bias)
    z = E.edited(row, (), bias)
    assert sorted(z[ids].tolist(), reverse=True) == [8 - 1 / 1024, 8 - 2 / 1024, 8 - 3 / 1024, 8 - 4 / 1024] and len({int(v.view(torch.int32)) >> 16 for v in z[ids + [4000]]}) == 1
    q, edge, p = E.law(z, 1.0, **filt)
    E.check_case(q, p, edge, ROWS * 4, min_kept=kept)
    assert int((q > 0).sum()) == kept
    d = _draws(hip, row, edits, 2, launches=4, temperature=1.0, **filt)
    assert int((torch.bincount(d.long(), minlength=V) > 0).sum()) == kept, "the kept count is exact"
    E.assert_law(d, q, p, edge, f"one bucket, {filt}")
    # a fractional bias that no bf16 holds: 0.3 on the four tokens moves them above 8.0 as fp32 keys with low bits set
    edits.set_bias(2, {t: 0.3 + c / 4096 for c, t in enumerate(ids)})
    z = E.edited(row, (), {t: 0.3 + c / 4096 for c, t in enumerate(ids)})
    q, edge, p = E.law(z, 1.0, top_k=3)
    d = _draws(hip, row, edits, 2, launches=4, temperature=1.0, top_k=3)
    assert int((q > 0).sum()) == 3 and set(d.tolist()) == set(ids[1:])
    E.assert_law(d, q, p, edge, "bias 0.3 + c / 4096, top_k 3")


# ---- 5. order ------------------------------------------------------------------------------------------------------------------------------
def test_bias_comes_before_the_penalties_and_a_ban_beats_a_bias(hip):
    row = (torch.rand(V, generator=torch.Generator().manual_seed(65)) - 2.0).bfloat16()      # everything else in [-2, -1]
    A, B, C = 100, 2000, 3000
    row[A], row[B] = 2.0, 3.0
    e, s = hip.logit_edits_create(1, V), hip.sampler_create(1, V)
    s.reset_slot(0, [A])                                       # A has history
    e.set_bias(0, {A: 3.0})
    pen = dict(repetition_penalty=2.0)
    z = E.edited(row, (), {A: 3.0}, prompt_ids=[A], **pen)      # bias then penalty: (2 + 3) / 2 = 2.5 < 3
    other = E.penalise(row, prompt_ids=[A], **pen)
    other[A] += 3.0                                            # penalty then bias: 2 / 2 + 3 = 4 > 3
    assert int(z.argmax()) == B and int(other.argmax()) == A and float(z[A]) == 2.5
    g = _draws(hip, row, e, 0, rows=64, launches=1, sampler=s, slot=0, temperature=0.0, **pen)
    assert bool((g == B).all()), "the kernel applies the bias first"
    # the sign test of the repetition penalty sees the biased value: -1.5 + 3 > 0 is divided, not multiplied
    row2 = row.clone()
    row2[A] = -1.5
    z2 = E.edited(row2, (), {A: 3.0}, prompt_ids=[A], **pen)
    assert float(z2[A]) == 0.75
    # a banned token with a +100 bias is never drawn; +-inf biases are honoured
    e.set_bias(0, {A: 100.0, C: float("inf")})
    e.ban(0, [A])
    assert bool((_draws(hip, row, e, 0, rows=64, launches=1, temperature=1.0) == C).all()), "+inf wins"
    e.ban(0, [C])
    d = _draws(hip, row, e, 0, rows=1024, launches=2, temperature=1.0)
    assert A not in d.tolist() and C not in d.tolist()
    e.ban(0, [A, C], False)
    e.set_bias(0, {B: float("-inf"), A: float("nan")})         # -inf removes B; a NaN bias counts as 0
    d = _draws(hip, row, e, 0, rows=1024, launches=2, temperature=1.0)
    assert B not in d.tolist() and float(e.read(0)[1][A]) == 0.0
    assert bool((_draws(hip, row, e, 0, rows=8, launches=1, temperature=0.0) == A).all())
    e.close()
    s.close()


# ---- 6. table edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab,n", [(V, 1), (V, 1024), (152064, 300)])
def test_bias_table_sizes(hip, vocab, n):
    row = _row(66, vocab=vocab, scale=1.0)
    g = torch.Generator().manual_seed(n)
    toks = sorted(torch.randperm(vocab, generator=g)[:n].tolist())
    vals = (torch.rand(n, generator=g) * 2 - 1).tolist()
    e = hip.logit_edits_create(2, vocab)
    for hit in sorted({0, n // 2, n - 1}):                    # the first, a middle and the last entry of the sorted table carry the winning bias
        bias = dict(zip(toks, vals))
        bias[toks[hit]] = 40.0
        items = list(bias.items())
        items = items[n // 3:] + items[:n // 3]                # handed over unsorted: the library sorts
        e.set_bias(1, items)
        got = e.read(1)[1].cpu()
        want = torch.zeros(vocab)
        want[torch.tensor(list(bias))] = torch.tensor(list(bias.values()), dtype=torch.float32)
        assert torch.equal(got, want)
        d = _draws(hip, row, e, 1, rows=64, launches=1, temperature=0.0)
        assert bool((d == toks[hit]).all()), (n, hit)
        d = _draws(hip, row, e, 1, rows=256, launches=1, temperature=1.0)      # p(other) ~ vocab x e^-37
        assert bool((d == toks[hit]).all())
    if vocab == V:
        bias = dict(zip(toks, vals))
        e.set_bias(1, bias)
        z = E.edited(row, (), bias)
        q, edge, p = E.law(z, 0.5, top_k=200)
        E.check_case(q, p, edge, ROWS * 4, min_kept=200)
        E.assert_law(_draws(hip, row, e, 1, launches=4, temperature=0.5, top_k=200), q, p, edge, f"{n} biased tokens, top_k 200")
    with pytest.raises(hip.ThinkDiffHipError, match="at most 1024"):
        e.set_bias(0, {t: 1.0 for t in range(1025)})
    with pytest.raises(hip.ThinkDiffHipError, match="given twice"):
        e.set_bias(0, [(5, 1.0), (9, 2.0), (5, 3.0)])
    with pytest.raises(hip.ThinkDiffHipError, match="outside the vocabulary"):
        e.set_bias(0, {vocab: 1.0})
    assert int(e.read(0)[1].count_nonzero()) == 0, "a refused call changes nothing"
    e.close()


# ---- 7. rows are independent -------------------------------------------------------------------------------------------------------------------
def test_rows_of_one_launch_are_independent(hip, edits):
    x = (torch.randn(8, V, generator=torch.Generator().manual_seed(67)) * 3).bfloat16().cuda()
    edits.reset_slot(0)
    edits.reset_slot(3)
    b0 = x[0].float().topk(30).indices.tolist() + x[4].float().topk(30).indices.tolist()
    b3 = x[5].float().topk(3).indices.tolist()
    edits.ban(0, b0)
    bias3 = {int(t): 6.0 for t in x[2].float().topk(400).indices[200:].tolist()}
    edits.set_bias(3, bias3)
    edits.ban(3, b3)
    slots = [0, -1, 3, 3, 0, 3, -1, 9]
    rows = [dict(temperature=0.6, top_p=0.9, seed=1, stream=0), dict(temperature=0.0, top_k=7, seed=2, stream=5),
            dict(temperature=1.0, top_k=40, seed=3, stream=1), dict(temperature=1.3, min_p=0.02, seed=4, stream=9),
            dict(temperature=0.0, seed=5, stream=2), dict(temperature=0.0, seed=6, stream=3),
            dict(temperature=2.0, top_p=0.5, seed=7, stream=4), dict(temperature=0.7, top_k=3, seed=8, stream=6)]
    for rep in range(3):
        o = [rep, 3 + rep, 1, 100, 7, 2, 5 + rep, 9]
        batch = hip.sample_rows_edit(x, rows, o, None, False, edits, slots)
        single = torch.cat([hip.sample_rows_edit(x[i:i + 1], [rows[i]], [o[i]], None, False, edits, [slots[i]]) for i in range(8)])
        assert torch.equal(batch, single)
        plain = hip.sample_rows(x, rows, o)
        assert all(int(batch[i]) == int(plain[i]) for i in (1, 6, 7)), "rows without an edit slot are sample_rows' rows"
        for i, b, bias in ((4, b0, None), (5, b3, bias3)):      # greedy rows: the first index of the largest edited logit
            z = E.edit(x[i].cpu(), b, bias)
            assert int(batch[i]) == int((z == z.max()).nonzero()[0])


# ---- 8. ban on, then off -------------------------------------------------------------------------------------------------------------------------
def test_clearing_a_ban_restores_the_unedited_ids_and_the_bias(hip, edits):
    x = (torch.randn(64, V, generator=torch.Generator().manual_seed(68)) * 3).bfloat16().cuda()
    rows = [dict(temperature=0.7, top_k=100, top_p=0.95, seed=5, stream=r) for r in range(64)]
    ref = hip.sample_rows(x, rows, 0)
    ids = sorted(set(ref.tolist()))                            # ban exactly what was drawn
    edits.reset_slot(0)
    edits.ban(0, ids)
    on = hip.sample_rows_edit(x, rows, 0, None, False, edits, 0)
    assert not (set(on.tolist()) & set(ids))
    edits.ban(0, ids, False)
    assert int(edits.read(0)[0].sum()) == 0
    assert torch.equal(hip.sample_rows_edit(x, rows, 0, None, False, edits, 0), ref)
    # a ban over a biased token, cleared: the bias is back
    row, T = _row(69), 0.8
    top = int(row.float().argmax())
    bias = {top: -2.5, 77: 4.0}
    edits.set_bias(0, bias)
    edits.ban(0, [top, 77, 1234])
    b, v = edits.read(0)
    assert b.cpu().nonzero().flatten().tolist() == sorted([top, 77, 1234]) and float(v[top]) == -2.5 and float(v[77]) == 4.0
    assert not ({top, 77, 1234} & set(_draws(hip, row, edits, 0, launches=1, temperature=T).tolist()))
    edits.ban(0, [top, 77, 1234], False)
    _check_law(hip, row, edits, 0, E.edited(row, (), bias), T, "ban cleared over biased tokens", min_kept=5)


# ---- 9. the engine -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(hip):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    return Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                               intermediate_size=1024, vocab_size=V), max_model_len=256, n_slots=4).init_random(3, std=0.05)


PROMPT = list(range(5, 25))


@pytest.fixture(scope="module")
def plain(engine):
    from thinkdiff.models.qwen2_vl import SamplingParams
    return engine.generate(PROMPT, SamplingParams(temperature=0.0, max_tokens=12, min_tokens=12))["token_ids"]


def test_engine_bad_words(hip, engine, plain):
    from thinkdiff.models.qwen2_vl import SamplingParams
    kw = dict(temperature=0.0, max_tokens=12, min_tokens=12)
    out = engine.generate(PROMPT, SamplingParams(bad_words_token_ids=[[plain[0]]], **kw))["token_ids"]
    assert len(out) == 12 and plain[0] not in out
    s = next(i for i in range(3, 11) if plain[i] not in plain[:i])      # (the word's first token must not have occurred earlier, or the ban would bite earlier)
    out = engine.generate(PROMPT, SamplingParams(bad_words_token_ids=[plain[s:s + 2]], **kw))["token_ids"]
    assert out[:s + 1] == plain[:s + 1] and out[s + 1] != plain[s + 1], (s, out, plain)
    assert all(out[i:i + 2] != plain[s:s + 2] for i in range(11))
    # the same through the batch entry, next to a request without edits
    outs = engine.generate_batch([{"prompt_token_ids": PROMPT}, {"prompt_token_ids": PROMPT}],
                                 [SamplingParams(bad_words_token_ids=[[plain[0]]], **kw), SamplingParams(**kw)])
    assert plain[0] not in outs[0]["token_ids"] and len(outs[0]["token_ids"]) == len(outs[1]["token_ids"]) == 12


def test_engine_min_tokens_mask(hip, engine, plain):
    from thinkdiff.models.qwen2_vl import SamplingParams
    stop = plain[2]
    kw = dict(temperature=0.0, max_tokens=12, min_tokens=8, stop_token_ids=[stop])
    on = engine.generate(PROMPT, SamplingParams(mask_stop_below_min_tokens=True, **kw))["token_ids"]
    assert len(on) >= 8 and stop not in on[:8] and (stop in plain[:2] or on[:2] == plain[:2])
    off = engine.generate(PROMPT, SamplingParams(**kw))["token_ids"]
    end = next((i for i in range(7, 12) if plain[i] == stop), 11)
    assert off == plain[:end + 1], "the default keeps today's rule: the stop id is sampled and only does not stop"


def test_engine_allowed_ids_and_slot_reuse(hip, engine, plain):
    from thinkdiff.models.qwen2_vl import SamplingParams
    allowed = list(range(100, 4000, 250))
    assert len(allowed) == 16
    kw = dict(temperature=0.0, max_tokens=10, min_tokens=10)
    out = engine.generate(PROMPT, SamplingParams(allowed_token_ids=allowed, **kw))["token_ids"]
    assert len(out) == 10 and set(out) <= set(allowed)
    out = engine.generate(PROMPT, SamplingParams(allowed_token_ids=allowed, temperature=1.0, top_p=1.0, seed=3, max_tokens=10, min_tokens=10))["token_ids"]
    assert len(out) == 10 and set(out) <= set(allowed)
    # generate_continuous: the second request takes over the slot of the first, which had edits, and samples plainly
    other = list(range(40, 60))
    alone = engine.generate_continuous([{"prompt_token_ids": other}], [SamplingParams(**kw)], max_live=1)[0]["token_ids"]
    outs = engine.generate_continuous([{"prompt_token_ids": PROMPT}, {"prompt_token_ids": other}],
                                      [SamplingParams(allowed_token_ids=allowed, logit_bias={allowed[3]: 50.0}, **kw), SamplingParams(**kw)], max_live=1)
    assert outs[0]["token_ids"] == [allowed[3]] * 10 and outs[1]["token_ids"] == alone
    with pytest.raises(ValueError, match="outside the vocabulary"):
        engine.generate(PROMPT, SamplingParams(allowed_token_ids=[5, V], **kw))
    with pytest.raises(ValueError, match="nothing could be sampled"):
        engine.generate(PROMPT, SamplingParams(allowed_token_ids=[5], bad_words_token_ids=[[5]], **kw))
