"""td_sample_rows_bf16 (per-row top-k, top-p, min-p, penalties, seed) on the GPU against the fp64 restatement of its rule in
tests/sampler_rows_common.py, under the statistical bars of tests/test_sampler_gpu.py, and the engine's per-request path end to end.

The kernel draws from its own counter-based stream, so a law is checked on N = 65 536 draws of one fixed row: 16 launches of 4096 rows that differ
only in `stream` / `offset`, the history read-only (update_state = 0).  Every case is first run through the restatement on the CPU (`check_case`):
the kept set has the size the case intends, E[TV] is finite, no token sits on the min-p threshold."""
import pytest
import torch

import sampler_rows_common as C

pytestmark = pytest.mark.gpu

V = 4096
ROWS, LAUNCHES = 4096, 16


def _row(seed, vocab=V, scale=3.0):
    return (torch.randn(vocab, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16()


def _draws(hip, row, rows=ROWS, launches=LAUNCHES, sampler=None, seed=1234, **fields):
    """rows x launches draws of one row: row r of launch o draws from (seed, o, r)."""
    logits = row.cuda()[None].expand(rows, row.numel()).contiguous()
    table = hip.pack_sample_rows([dict(fields, seed=seed, stream=r) for r in range(rows)]).cuda()
    out = [hip.sample_rows(logits, table, torch.full((rows,), o, dtype=torch.int64, device="cuda"), sampler, False) for o in range(launches)]
    torch.cuda.synchronize()
    out = torch.cat(out)
    assert out.dtype == torch.int32
    return out.cpu()


# ---- 1. regression anchor --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [152064, 4096])
def test_everything_off_is_sample_top_p_bit_for_bit(hip, vocab):
    x = (torch.randn(64, vocab, generator=torch.Generator().manual_seed(vocab)) * 3).bfloat16().cuda()
    for temperature, top_p in ((0.6, 0.9), (1.0, 1.0), (0.0, 0.9)):
        for off in range(4):
            ref = hip.sample_top_p(x, temperature, top_p, seed=77, offset=off)
            offs = torch.full((64,), off, dtype=torch.int64, device="cuda")
            for extra in ({}, dict(top_k=vocab, min_p=0.0), dict(top_k=0)):
                got = hip.sample_rows(x, [dict(extra, temperature=temperature, top_p=top_p, seed=77, stream=r, slot=-1) for r in range(64)], offs)
                assert torch.equal(got, ref), (temperature, top_p, off, extra)


# ---- 2. top-k -----------------------------------------------------------------------------------------------------------------------------
def test_top_k_1_is_argmax(hip):
    row = _row(21)
    d = _draws(hip, row, launches=2, temperature=1.0, top_k=1)
    assert bool((d == int(row.float().argmax())).all())


@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_top_k_law_and_top_p_of_the_top_k_mass(hip, top_p):
    row, T = _row(22), 0.8
    q, edge, p = C.law(C.penalise(row), T, top_k=50, top_p=top_p)
    C.check_case(q, p, edge, ROWS * LAUNCHES, min_kept=50 if top_p == 1.0 else 5)
    if top_p < 1.0:      # the order is visible: top-p of the whole mass would keep another set
        assert int((q > 0).sum()) < 50 and int((q > 0).sum()) != int((C.law(C.penalise(row), T, top_p=top_p)[0] > 0).sum())
    C.assert_law(_draws(hip, row, temperature=T, top_k=50, top_p=top_p), q, p, edge, f"top_k 50 top_p {top_p}")


def test_top_k_boundary_tie_keeps_exactly_k_tokens_worth(hip):
    row, T = _row(23), 0.8
    order = torch.argsort(row.float(), descending=True, stable=True)
    row[order[44:60]] = row[order[44]].clone()                   # the 45th .. 60th largest are equal: the k = 50 boundary cuts through the tie
    q, edge, p = C.law(C.penalise(row), T, top_k=50)
    C.check_case(q, p, edge, ROWS * LAUNCHES, min_kept=50)
    tie = (p - edge).abs() <= 1e-12 * edge
    assert int(tie.sum()) == 16 and int((q > 0).sum()) == 50 and int(((q > 0) & tie).sum()) == 6
    d = _draws(hip, row, temperature=T, top_k=50)
    C.assert_law(d, q, p, edge, "top_k 50, tie at the boundary")
    counts = torch.bincount(d.long(), minlength=V)
    assert int(((counts > 0) & tie).sum()) == 6, "6 of the 16 tied tokens complete the 50"


def test_top_k_law_full_vocabulary(hip):
    row, T = _row(24, vocab=152064), 0.8
    q, edge, p = C.law(C.penalise(row), T, top_k=50)
    C.check_case(q, p, edge, 1024 * 16, min_kept=50)
    C.assert_law(_draws(hip, row, rows=1024, temperature=T, top_k=50), q, p, edge, "vocab 152064 top_k 50")


# ---- 3. min-p -----------------------------------------------------------------------------------------------------------------------------
def test_min_p_law(hip):
    row, T = _row(31), 1.0
    q, edge, p = C.law(C.penalise(row), T, min_p=0.05)
    C.check_case(q, p, edge, ROWS * LAUNCHES, min_kept=3, min_p=0.05)
    assert int((q > 0).sum()) < 200
    C.assert_law(_draws(hip, row, temperature=T, min_p=0.05), q, p, edge, "min_p 0.05")


def test_min_p_1_keeps_only_the_maximum(hip):
    row = _row(32)
    top = row.float().max()
    row[100] = row[3000] = top                                 # three indices hold the maximum
    d = _draws(hip, row, launches=2, temperature=1.0, min_p=1.0)
    assert bool((row[d.long()].float() == top).all()) and len(set(d.tolist())) == 3


def test_min_p_top_p_top_k_intersection(hip):
    row, T = _row(33), 1.5
    kw = dict(top_k=100, top_p=0.9, min_p=0.1)
    q, edge, p = C.law(C.penalise(row), T, **kw)
    C.check_case(q, p, edge, ROWS * LAUNCHES, min_kept=3, min_p=0.1)
    # every filter bites: the intersection is smaller than what top-k + top-p alone keep, and than what min-p alone keeps
    n = int((q > 0).sum())
    assert n < int((C.law(C.penalise(row), T, top_k=100, top_p=0.9)[0] > 0).sum()) and n <= int((C.law(C.penalise(row), T, min_p=0.1)[0] > 0).sum())
    C.assert_law(_draws(hip, row, temperature=T, **kw), q, p, edge, "top_k 100 top_p 0.9 min_p 0.1")


# ---- 4. penalties ----------------------------------------------------------------------------------------------------------------------------
def _history(row):
    """~40 history tokens: the row maximum, the next three, six tokens with negative logits, 30 spread ones; prompt-only, generated-only and both;
    one count of 7."""
    order = torch.argsort(row.float(), descending=True, stable=True)
    neg = [int(t) for t in order if float(row[t]) < 0][:3] + [int(order[-1]), int(order[-2]), int(order[-500])]
    ids = [int(order[0]), int(order[1]), int(order[2]), int(order[3])] + neg + [int(order[i]) for i in range(10, 310, 10)]
    assert len(set(ids)) == 40
    prompt = ids[0:1] + ids[4:7] + ids[10:25] + [V + 5, -1]           # (two ids outside the vocabulary: ignored)
    counts = torch.zeros(V, dtype=torch.int32)
    for j, t in enumerate(ids[1:4] + ids[7:10] + ids[20:40]):
        counts[t] = 1 + j % 3
    counts[ids[1]] = 7
    return prompt, counts


@pytest.fixture(scope="module")
def penalty_state(hip):
    row = _row(41)
    prompt, counts = _history(row)
    s = hip.sampler_create(2, V)
    s.reset_slot(1, prompt)
    s.set_counts(1, counts)
    torch.cuda.synchronize()
    yield row, prompt, counts, s
    s.close()


@pytest.mark.parametrize("name,pen,filt", [
    ("repetition 1.3", dict(repetition_penalty=1.3), {}),
    ("presence 1.5 + frequency 0.5", dict(presence_penalty=1.5, frequency_penalty=0.5), {}),
    ("all three, top_k 50, top_p 0.9", dict(repetition_penalty=1.3, presence_penalty=1.5, frequency_penalty=0.5), dict(top_k=50, top_p=0.9)),
    ("the maximum demoted", dict(repetition_penalty=2.0, presence_penalty=1.0, frequency_penalty=0.25), {}),
])
def test_penalty_law(hip, penalty_state, name, pen, filt):
    row, prompt, counts, s = penalty_state
    T = 0.8
    z = C.penalise(row, prompt, counts, **pen)
    q, edge, p = C.law(z, T, **filt)
    C.check_case(q, p, edge, ROWS * LAUNCHES, min_kept=5)
    assert not torch.equal(z, row.float())
    if "demoted" in name:
        assert int(z.argmax()) != int(row.float().argmax())
        g = _draws(hip, row, rows=64, launches=1, sampler=s, slot=1, temperature=0.0, **pen)
        assert bool((g == int(z.argmax())).all()), "greedy takes the maximum AFTER the penalties"
    C.assert_law(_draws(hip, row, sampler=s, slot=1, temperature=T, **pen, **filt), q, p, edge, name)


@pytest.mark.parametrize("filt,kept", [(dict(top_k=2), 2), (dict(top_k=3, top_p=0.9), 3), (dict(top_k=5), 5), (dict(top_p=0.4), 3), (dict(min_p=0.9995), 1)])
def test_boundary_among_penalised_tokens_of_one_bf16_bucket(hip, filt, kept):
    """Four penalised tokens whose fp32 values differ only below bf16 precision (8 - c / 1024, c = 1 .. 4) and an unpenalised 7.96875 share one
    16-bit key bucket, and every boundary falls inside it: the third and fourth radix levels order them."""
    row = _row(45, scale=1.0)
    ids = [500, 1500, 2500, 3500]
    row[ids] = 8.0
    row[4000] = 7.96875
    counts = torch.zeros(V, dtype=torch.int32)
    counts[ids] = torch.tensor([3, 1, 4, 2], dtype=torch.int32)
    s = hip.sampler_create(1, V)
    s.set_counts(0, counts)
    pen = dict(frequency_penalty=1.0 / 1024)
    z = C.penalise(row, (), counts, **pen)
    assert sorted(z[ids].tolist(), reverse=True) == [8 - 1 / 1024, 8 - 2 / 1024, 8 - 3 / 1024, 8 - 4 / 1024] and len({int(v.view(torch.int32)) >> 16 for v in z[ids + [4000]]}) == 1
    q, edge, p = C.law(z, 1.0, **filt)
    C.check_case(q, p, edge, ROWS * 4, min_kept=kept, min_p=filt.get("min_p", 0.0))
    assert int((q > 0).sum()) == kept
    d = _draws(hip, row, launches=4, sampler=s, slot=0, temperature=1.0, **pen, **filt)
    if kept == 1:
        assert bool((d == 1500).all())
    else:
        C.assert_law(d, q, p, edge, f"one bucket, {filt}")
    s.close()


def test_penalties_without_a_slot_or_switched_off_change_nothing(hip, penalty_state):
    row, _, _, s = penalty_state
    x = row.cuda()[None].expand(64, V).contiguous()
    offs = torch.zeros(64, dtype=torch.int64, device="cuda")
    ref = hip.sample_top_p(x, 0.7, 0.95, seed=5, offset=0)
    base = dict(temperature=0.7, top_p=0.95, seed=5)
    a = hip.sample_rows(x, [dict(base, stream=r, slot=-1, repetition_penalty=1.5, presence_penalty=1.0) for r in range(64)], offs, s)
    b = hip.sample_rows(x, [dict(base, stream=r, slot=1) for r in range(64)], offs, s)
    c = hip.sample_rows(x, [dict(base, stream=r, slot=7, repetition_penalty=1.5) for r in range(64)], offs, s)      # a slot the state does not have
    d = hip.sample_rows(x, [dict(base, stream=r, slot=1, repetition_penalty=float("nan"), presence_penalty=float("inf"), top_p=7.0) for r in range(64)], offs, s)
    assert torch.equal(a, ref) and torch.equal(b, ref) and torch.equal(c, ref)
    assert torch.equal(d, hip.sample_top_p(x, 0.7, 1.0, seed=5, offset=0))
    with pytest.raises(hip.ThinkDiffHipError, match="differs from the sampler state"):
        hip.sample_rows(torch.zeros(1, 1024, dtype=torch.bfloat16, device="cuda"), [dict()], 0, s)


# ---- 5. per-row parameters -------------------------------------------------------------------------------------------------------------------
def test_rows_of_one_launch_are_independent(hip):
    x = (torch.randn(8, V, generator=torch.Generator().manual_seed(51)) * 3).bfloat16().cuda()
    rows = [dict(temperature=0.6, top_p=0.9, seed=1, stream=0), dict(temperature=0.0, top_k=7, seed=2, stream=5),
            dict(temperature=1.0, top_k=40, seed=3, stream=1), dict(temperature=1.3, min_p=0.02, seed=4, stream=9),
            dict(temperature=0.0, seed=5, stream=2), dict(temperature=0.9, top_k=200, top_p=0.8, min_p=0.01, seed=2 ** 63 + 11, stream=3),
            dict(temperature=2.0, top_p=0.5, seed=7, stream=4), dict(temperature=0.7, top_k=3, seed=8, stream=6)]
    offs = [0, 3, 1, 100, 7, 2 ** 40, 5, 9]
    for rep in range(3):
        o = [v + rep for v in offs]
        batch = hip.sample_rows(x, rows, o)
        single = torch.cat([hip.sample_rows(x[i:i + 1], [rows[i]], [o[i]]) for i in range(8)])
        assert torch.equal(batch, single)
        assert int(batch[1]) == int(x[1].float().argmax()) and int(batch[4]) == int(x[4].float().argmax())
    # the draw is a function of (seed, offset, stream) only
    again = hip.sample_rows(x[[2, 2, 2, 2]].contiguous(), [rows[2], dict(rows[2], stream=2), dict(rows[2], seed=4), rows[2]], [1, 1, 1, 1])
    assert int(again[0]) == int(again[3]) == int(hip.sample_rows(x[2:3], [rows[2]], [1]))
    many = hip.sample_rows(x[[2] * 64].contiguous(), [dict(rows[2], stream=r) for r in range(64)], 1)
    assert len(set(many.tolist())) > 8


# ---- 6. state updates --------------------------------------------------------------------------------------------------------------------------
def test_update_state_counts_what_was_sampled(hip):
    s = hip.sampler_create(4, V)
    g = torch.Generator().manual_seed(61)
    prompts = [torch.randint(0, V, (n,), generator=g).tolist() for n in (5, 40, 1, 300)]
    for slot, p in enumerate(prompts):
        s.reset_slot(slot, p + [V, -3])
    x = (torch.randn(4, V, generator=g) * 3).bfloat16().cuda()
    rows = [dict(temperature=1.0, top_k=20, slot=sl, stream=sl, seed=9, frequency_penalty=0.3 if sl == 1 else 0.0) for sl in range(4)]
    table = hip.pack_sample_rows(rows).cuda()
    ids = torch.stack([hip.sample_rows(x, table, torch.full((4,), t, dtype=torch.int64, device="cuda"), s, True) for t in range(200)]).cpu()      # [200, 4]
    for sl in range(4):
        assert torch.equal(s.read_counts(sl).cpu().long(), torch.bincount(ids[:, sl].long(), minlength=V))
        mask = torch.zeros(V, dtype=torch.uint8)
        mask[torch.tensor(prompts[sl])] = 1
        assert torch.equal(s.read_prompt_mask(sl).cpu(), mask)
    # a row without a slot leaves every count as it is; update_state = 0 too
    before = [s.read_counts(sl).clone() for sl in range(4)]
    hip.sample_rows(x, [dict(r, slot=-1) for r in rows], 0, s, True)
    hip.sample_rows(x, table, torch.zeros(4, dtype=torch.int64, device="cuda"), s, False)
    assert all(torch.equal(s.read_counts(sl), before[sl]) for sl in range(4))
    # resetting slot 2 zeroes slot 2 only
    s.reset_slot(2, [11, 12])
    assert int(s.read_counts(2).sum()) == 0 and s.read_prompt_mask(2).nonzero().flatten().tolist() == [11, 12]
    assert all(torch.equal(s.read_counts(sl), before[sl]) for sl in (0, 1, 3)) and int(before[3].sum()) == 200
    # counts saturate at 65 535
    c = torch.zeros(V, dtype=torch.int32)
    c[77] = 65535
    c[78] = 65534
    s.set_counts(0, c)
    y = torch.full((1, V), -30.0).bfloat16()
    y[0, 77] = y[0, 78] = 5.0
    for t in range(4):
        hip.sample_rows(y.cuda(), [dict(temperature=1.0, slot=0, seed=1)], t, s, True)
    got = s.read_counts(0).cpu()
    assert int(got[77]) == 65535 and int(got[78]) in (65534, 65535) and int(got.sum()) == int(got[77]) + int(got[78]), "saturates, never wraps"
    with pytest.raises(hip.ThinkDiffHipError, match="slot 4"):
        s.reset_slot(4, [1])
    s.close()


# ---- 7. degenerate rows, a penalised history present ------------------------------------------------------------------------------------------------
def test_degenerate_rows_with_history_always_yield_a_token(hip):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, V, generator=g).bfloat16()
    x[0, 777] = float("inf")
    x[1, 12] = float("inf"); x[1, 3000] = float("inf")
    x[2, :] = float("-inf")
    x[3, :] = float("nan")
    x[4, :] = float("-inf"); x[4, 99] = 1.5
    x[5, :] = float("-inf"); x[5, 200] = -2.0; x[5, 300] = float("nan")
    s = hip.sampler_create(1, V)
    s.reset_slot(0, [777, 12, 99, 200, 5, 6, 7])
    c = torch.zeros(V, dtype=torch.int32)
    c[777], c[99], c[3000], c[200] = 3, 2, 1, 4
    s.set_counts(0, c)
    for pen in (dict(repetition_penalty=1.5, presence_penalty=1.0, frequency_penalty=0.5), dict(repetition_penalty=0.5, presence_penalty=-2.0)):
        for T, extra in ((0.6, dict(top_p=0.9)), (1.0, dict(top_k=5, min_p=0.2)), (0.0, {})):
            for o in range(3):
                ids = hip.sample_rows(x.cuda(), [dict(pen, temperature=T, slot=0, stream=r, seed=3, **extra) for r in range(6)], o, s, False).cpu()
                assert all(0 <= int(i) < V for i in ids), ids
                assert int(ids[0]) == 777 and int(ids[1]) == 12 and int(ids[4]) == 99 and int(ids[5]) == 200, (pen, T, ids)
    s.close()


# ---- 8. the engine ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(hip):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    return Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                               intermediate_size=1024, vocab_size=V), max_model_len=256, n_slots=4).init_random(3, std=0.05)


def test_engine_seeded_requests_do_not_depend_on_their_batch(hip, engine):
    """A request with its own seed draws from (seed, its token count, 0): its tokens depend on neither the call's key nor the rows it shares a step
    with -- PROVIDED its logits agree bit for bit.  Decode does (the batch of 1 and the batch of 3 take the same M <= 4 weight-stream kernel, whose
    M-independence tests/test_qwen2_gpu.py asserts), but the PREFILL does not: measured on this engine, the logits of the third prompt of a packed
    prefill pass differ from those of the same prompt prefilled alone in 2728 of 4096 entries (up to one bf16 step; the packed pass runs its GEMMs and
    attention at another M), and a draw over a min-p set of thousands of nearly flat logits moves with them.  So a seeded request is compared between
    generate_batch calls that present it in different orders and rows (the same packed shapes, so the same logits), and between generate and a
    generate_batch of one, which share the prefill."""
    from thinkdiff.models.qwen2_vl import SamplingParams
    prompts = [list(range(5, 25)), list(range(40, 60)), list(range(100, 120))]
    sps = [SamplingParams(temperature=0.7, top_p=0.9, top_k=1, max_tokens=10, min_tokens=10),
           SamplingParams(temperature=0.8, top_p=0.95, top_k=40, seed=1234, max_tokens=12, min_tokens=12, repetition_penalty=1.1),
           SamplingParams(temperature=1.0, top_p=1.0, min_p=0.05, seed=99, max_tokens=8, min_tokens=8)]

    def batch(order, key):
        torch.manual_seed(key)                            # (the call's key does not enter a seeded request's draw)
        out = engine.generate_batch([{"prompt_token_ids": prompts[i]} for i in order], [sps[i] for i in order])
        return {i: o["token_ids"] for i, o in zip(order, out)}

    a, b, c = batch([0, 1, 2], 0), batch([2, 0, 1], 1), batch([1, 2, 0], 2)
    assert [len(a[i]) for i in range(3)] == [10, 12, 8]
    greedy = engine.generate(prompts[0], SamplingParams(temperature=0.0, max_tokens=10, min_tokens=10))["token_ids"]
    assert a[0] == greedy == b[0] == c[0], "top_k = 1 is greedy"
    for i in (1, 2):
        assert a[i] == b[i] == c[i], f"request {i} (seed {sps[i].seed}) depends on its place in the batch"
        torch.manual_seed(1000 + i)
        alone = engine.generate(prompts[i], sps[i])["token_ids"]
        torch.manual_seed(2000 + i)
        assert alone == engine.generate_batch([{"prompt_token_ids": prompts[i]}], [sps[i]])[0]["token_ids"]
    other = batch([0, 1, 2], 0)
    assert other == a
    sps[1] = SamplingParams(**{**sps[1].__dict__, "seed": 1235})
    assert batch([0, 1, 2], 0)[1] != a[1], "another seed, other tokens"


def test_engine_repetition_penalty_forbids_repeats(hip, engine):
    from thinkdiff.models.qwen2_vl import SamplingParams
    prompt = list(range(60, 80))                          # (chosen on the GPU: plain greedy repeats four tokens on it)
    plain = engine.generate(prompt, SamplingParams(temperature=0.0, max_tokens=32, min_tokens=32))["token_ids"]
    assert len(set(plain) | set(prompt)) < len(plain) + len(prompt), "plain greedy repeats on this prompt (the case needs it to)"
    pen = engine.generate(prompt, SamplingParams(temperature=0.0, max_tokens=32, min_tokens=32, repetition_penalty=1e4))["token_ids"]
    assert len(pen) == 32 and len(set(pen) | set(prompt)) == 32 + len(prompt), "a token of the prompt or the output came again"
    assert engine._sampler_state().read_counts(0).sum().item() == 32
    assert engine._sampler_state().read_prompt_mask(0).nonzero().flatten().tolist() == prompt
    # the same through the continuous scheduler, two requests sharing steps, and the history of a reused slot starts over
    sp = SamplingParams(temperature=0.0, max_tokens=32, min_tokens=32, repetition_penalty=1e4)
    outs = engine.generate_continuous([{"prompt_token_ids": prompt}, {"prompt_token_ids": list(range(200, 210))}, {"prompt_token_ids": prompt}], sp, max_live=2)
    for o, pr in zip(outs, (prompt, list(range(200, 210)), prompt)):      # (no comparison with `pen`: a packed prefill's logits may differ by a bf16 step)
        assert len(o["token_ids"]) == 32 and len(set(o["token_ids"]) | set(pr)) == 32 + len(pr)
    st = engine._sampler_state()      # the third request took over slot 0: had its history not been reset, the slot would count 64 tokens
    assert int(st.read_counts(0).sum()) == 32 == int(st.read_counts(1).sum()) and st.read_prompt_mask(0).nonzero().flatten().tolist() == prompt


def test_engine_default_sampling_is_still_reproducible_under_torch_seed(hip, engine):
    from thinkdiff.models.qwen2_vl import SamplingParams
    sp = SamplingParams(temperature=0.6, top_p=0.9, max_tokens=12, min_tokens=12)
    outs = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)
        outs.append(engine.generate(list(range(5, 25)), sp)["token_ids"])
    assert outs[0] == outs[1] and outs[0] != outs[2] and len(outs[0]) == 12
    a = engine.generate(list(range(5, 25)), sp, generator=torch.Generator().manual_seed(99))["token_ids"]
    b = engine.generate(list(range(5, 25)), sp, generator=torch.Generator().manual_seed(99))["token_ids"]
    assert a == b
    # a list of default SamplingParams goes through td_sample_rows_bf16 and draws what the single form draws (one key, stream = live row)
    torch.manual_seed(11)
    c = engine.generate(list(range(5, 25)), [sp])["token_ids"]
    assert c == outs[0]
