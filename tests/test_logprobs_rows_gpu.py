"""td_logprobs_rows_bf16 (the chosen token's logprob and rank and the top-n logprobs of rows of RAW bf16 logits) on the GPU against fp64
log_softmax and a stable sort (tests/logit_edits_common.py), and the engine's `logprobs` output end to end.

The bar LOGPROB_BAR = 2e-5 on |lp - lp64| for |lp| <= 64 is derived, not tuned: the fp32 ulp below 64 is 3.8e-6, the truncation of a 2^-40 fixed-point
sum is below V x 2^-40 = 1.4e-7, exp2 / log2 are 1-ulp operations."""
import pytest
import torch

import logit_edits_common as E

pytestmark = pytest.mark.gpu

BAR = E.LOGPROB_BAR


def _rows(vocab, rows=64, seed=0):
    return (torch.randn(rows, vocab, generator=torch.Generator().manual_seed(seed + vocab)) * 3).bfloat16()


@pytest.fixture(scope="module")
def big():
    """64 rows of 152 064 N(0, 3) bf16 logits (full of ties), their fp64 logprobs and stable descending order, computed once."""
    x = _rows(152064)
    lp64 = torch.log_softmax(x.double(), dim=-1)
    order = torch.sort(x.double(), dim=-1, descending=True, stable=True).indices
    return x, lp64, order


def _ids(x, seed=1):
    """Chosen tokens: random ones, the row maximum in row 0, the row minimum in row 1."""
    ids = torch.randint(0, x.shape[1], (x.shape[0],), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    ids[0], ids[1] = int(x[0].float().argmax()), int(x[1].float().argmin())
    return ids


# ---- 1. against fp64 log_softmax -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [4096, 152064])
def test_logprobs_match_fp64_log_softmax(hip, big, vocab):
    x, lp64 = (big[0], big[1]) if vocab == 152064 else (_rows(vocab), None)
    if lp64 is None:
        lp64 = torch.log_softmax(x.double(), dim=-1)
    ids = _ids(x)
    lp, rank, tid, tlp = (t.cpu() for t in hip.logprobs_rows(x.cuda(), ids, 20))
    ref = lp64.gather(1, ids.long()[:, None])[:, 0]
    assert bool((ref.abs() <= 64).all())
    err = float((lp.double() - ref).abs().max())
    err_top = float((tlp.double() - lp64.gather(1, tid.long())).abs().max())
    print(f"vocab {vocab}: max |lp - lp64| chosen {err:.3e}, top-20 {err_top:.3e} (bar {BAR:.0e})")
    assert err <= BAR and err_top <= BAR
    assert not bool(torch.isnan(lp).any() | torch.isnan(tlp).any())


# ---- 2. top ids and rank, exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 5, 20])
def test_top_ids_equal_a_stable_sort_and_rank_is_exact(hip, big, n):
    x, lp64, order = big
    ids = _ids(x, seed=2 + n)
    lp, rank, tid, tlp = (t.cpu() for t in hip.logprobs_rows(x.cuda(), ids, n, top_cap=20))
    assert tid.shape == (64, 20) and tlp.shape == (64, 20)
    assert torch.equal(tid[:, :n].long(), order[:, :n]), "descending value, then ascending index"
    assert bool((tid[:, n:] == -1).all()) and bool((tlp[:, n:] == float("-inf")).all()), "unused columns hold id -1 and lp -inf"
    if n >= 5:      # the case is what it claims: ties inside the top n of some row, so the index order decides
        top = x.float().gather(1, order[:, :n])
        assert bool((top[:, 1:] == top[:, :-1]).any())
    chosen = x.float().gather(1, ids.long()[:, None])
    assert torch.equal(rank.long(), (x.float() >= chosen).sum(-1))
    assert int(rank[0]) >= 1 and int(rank[1]) == 152064
    # top_cap below 20, and mixed n in one launch
    mixed = torch.tensor([(r % 7) - 1 for r in range(64)], dtype=torch.int32)
    lp2, rank2, tid2, _ = (t.cpu() for t in hip.logprobs_rows(x.cuda(), ids, mixed, top_cap=5))
    for r in range(64):
        m = int(mixed[r])
        if m >= 0:
            assert tid2[r, :m].tolist() == order[r, :m].tolist() and bool((tid2[r, m:] == -1).all())
            assert float(lp2[r]) == float(lp[r]) and int(rank2[r]) == int(rank[r]), "the chosen token's values do not depend on n"


# ---- 3. every token counts ----------------------------------------------------------------------------------------------------------------------
def test_every_position_enters_the_sum(hip):
    vocab = 2 * 8 * 1024 + 24                                 # (an odd number of 16-byte chunks, more than two sweeps of the 1024 threads)
    pos = [0, 7, 8, 8 * 1024 - 1, 8 * 1024, vocab - 1]
    x = torch.full((len(pos), vocab), -30.0).bfloat16()
    for r, j in enumerate(pos):
        x[r, j] = 0.0
    lp64 = torch.log_softmax(x.double(), dim=-1)
    ids = torch.tensor(pos, dtype=torch.int32)
    lp, rank, tid, tlp = (t.cpu() for t in hip.logprobs_rows(x.cuda(), ids, 2))
    # dropping position j would move lse from ~0 to -30 + ln(vocab - 1) = -20.3
    assert float((lp.double() - lp64.gather(1, ids.long()[:, None])[:, 0]).abs().max()) <= BAR
    assert rank.tolist() == [1] * len(pos) and tid[:, 0].tolist() == pos
    assert tid[:, 1].tolist() == [1, 0, 0, 0, 0, 0], "the first of the tied -30s"
    assert float((tlp[:, :2].double() - lp64.gather(1, tid[:, :2].long())).abs().max()) <= BAR
    other = torch.tensor([5] * len(pos), dtype=torch.int32)
    lp_o, rank_o, _, _ = (t.cpu() for t in hip.logprobs_rows(x.cuda(), other, 0, top_cap=0))
    assert float((lp_o.double() - lp64[:, 5]).abs().max()) <= BAR and rank_o.tolist() == [vocab] * len(pos)


# ---- 4. skips, degenerate rows, position independence -----------------------------------------------------------------------------------------------
def test_skipped_rows_are_untouched_and_degenerate_rows_never_give_nan(hip):
    V = 4096
    x = _rows(V, rows=8, seed=4)
    x[0, 777] = float("inf")
    x[1, 12] = float("inf"); x[1, 3000] = float("inf")
    x[2, :] = float("-inf")
    x[3, :] = float("nan")
    x[4, :] = float("-inf"); x[4, 99] = 1.5
    x[5, 300] = float("nan")
    ids = torch.tensor([777, 5, 9, 9, 99, 300, V, -1], dtype=torch.int32)
    n_top = torch.tensor([3, 3, 3, 3, 3, 3, 3, -1], dtype=torch.int32)
    sentinel = (torch.full((8,), 7.5, device="cuda"), torch.full((8,), 42, dtype=torch.int32, device="cuda"),
                torch.full((8, 4), 42, dtype=torch.int32, device="cuda"), torch.full((8, 4), 7.5, device="cuda"))
    lp, rank, tid, tlp = (t.cpu() for t in hip.logprobs_rows(x.cuda(), ids, n_top, top_cap=4, out=sentinel))
    inf = float("inf")
    assert not bool(torch.isnan(lp).any() | torch.isnan(tlp).any())
    assert (float(lp[7]), int(rank[7]), tid[7].tolist(), tlp[7].tolist()) == (7.5, 42, [42] * 4, [7.5] * 4), "n_top = -1: outputs untouched"
    assert (float(lp[0]), int(rank[0]), tid[0, 0].item(), float(tlp[0, 0]), float(tlp[0, 1])) == (0.0, 1, 777, 0.0, -inf), "+inf: those tokens 0, the others -inf"
    assert (float(lp[1]), int(rank[1]), tid[1, :2].tolist(), tlp[1, :3].tolist()) == (-inf, int((x[1].float() >= x[1, 5].float()).sum()), [12, 3000], [0.0, 0.0, -inf])
    for r in (2, 3):      # no finite value: every lp -inf, rank = vocab, the top ids are the first indices
        assert (float(lp[r]), int(rank[r]), tid[r, :3].tolist(), tlp[r, :3].tolist()) == (-inf, V, [0, 1, 2], [-inf] * 3)
    assert abs(float(lp[4])) <= BAR and abs(float(tlp[4, 0])) <= BAR, "one finite value has all the mass"
    assert (int(rank[4]), tid[4, :2].tolist(), float(tlp[4, 1])) == (1, [99, 0], -inf)
    assert (float(lp[5]), int(rank[5])) == (-inf, V), "a NaN logit counts as -inf"
    assert (float(lp[6]), int(rank[6])) == (-inf, 0) and int(tid[6, 0]) == int(x[6].float().argmax()), "an id outside the vocabulary: lp -inf, rank 0"
    assert bool((tid[:7, 3] == -1).all()) and bool((tlp[:7, 3] == -inf).all())
    # the same row at index 0 of a 1-row launch and at index 200 of a 256-row launch: equal bits
    big = _rows(152064, rows=1, seed=9)
    many = torch.zeros(256, 152064, dtype=torch.bfloat16)
    many[::3] = 1.0
    many[200] = big[0]
    one = hip.logprobs_rows(big.cuda(), [31], 20)
    all_ = hip.logprobs_rows(many.cuda(), [31] * 256, 20)
    for a, b in zip(one, all_):
        assert torch.equal(a[0].cpu().view(torch.int32), b[200].cpu().view(torch.int32))


# ---- 5. the engine -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(hip):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    return Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                               intermediate_size=1024, vocab_size=4096), max_model_len=256, n_slots=4).init_random(3, std=0.05)


def _step_logits(engine, prompt, toks):
    """The engine's own logits in front of every token of `toks` (generate()'s loop, teacher-forced), as fp64 log_softmax rows."""
    _, logits = engine.forward(engine.text_position_ids(len(prompt)), torch.tensor(prompt, dtype=torch.int32), None, 0, True, True)
    rows = []
    for step, t in enumerate(toks):
        rows.append(torch.log_softmax(logits.double().cpu().reshape(-1), dim=-1))
        _, lg = engine.decode_batch([t], [[len(prompt) + step]] * 3, [len(prompt) + step])
        logits = lg[0]
    return rows


def test_engine_greedy_logprobs(hip, engine):
    from thinkdiff.models.qwen2_vl import Logprob, SamplingParams
    prompt = list(range(5, 25))
    plain = engine.generate(prompt, SamplingParams(temperature=0.0, max_tokens=12, min_tokens=12))
    assert "logprobs" not in plain and "cumulative_logprob" not in plain
    out = engine.generate(prompt, SamplingParams(temperature=0.0, max_tokens=12, min_tokens=12, logprobs=5))
    assert out["token_ids"] == plain["token_ids"], "logprobs do not change what is sampled"
    ref = _step_logits(engine, prompt, out["token_ids"])
    assert len(out["logprobs"]) == 12
    worst = 0.0
    for d, t, lp64 in zip(out["logprobs"], out["token_ids"], ref):
        assert len(d) == 5 and next(iter(d)) == t and d[t].rank == 1 and isinstance(d[t], Logprob), "greedy: the chosen token is the first of the top 5"
        assert [v.rank for v in d.values()] == [1, 2, 3, 4, 5] and list(d) == torch.sort(lp64, descending=True, stable=True).indices[:5].tolist()
        worst = max(worst, max(abs(v.logprob - float(lp64[k])) for k, v in d.items()))
    print(f"engine: max |lp - lp64| over 12 x 5 logprobs {worst:.3e}")
    assert worst <= BAR
    assert abs(out["cumulative_logprob"] - sum(float(r[t]) for r, t in zip(ref, out["token_ids"]))) <= 12 * BAR
    # the batch and the continuous entries return the same structure
    sp = SamplingParams(temperature=0.0, max_tokens=6, min_tokens=6, logprobs=2)
    for outs in (engine.generate_batch([{"prompt_token_ids": prompt}, {"prompt_token_ids": list(range(40, 60))}], [sp, SamplingParams(temperature=0.0, max_tokens=6, min_tokens=6)]),
                 engine.generate_continuous([{"prompt_token_ids": prompt}, {"prompt_token_ids": list(range(40, 60))}], [sp, SamplingParams(temperature=0.0, max_tokens=6, min_tokens=6)], max_live=2)):
        assert len(outs[0]["logprobs"]) == 6 and "logprobs" not in outs[1]
        assert all(next(iter(d)) == t and d[t].rank == 1 and len(d) == 2 for d, t in zip(outs[0]["logprobs"], outs[0]["token_ids"]))
        assert abs(outs[0]["cumulative_logprob"] - sum(d[t].logprob for d, t in zip(outs[0]["logprobs"], outs[0]["token_ids"]))) < 1e-9


def test_engine_scores_a_forced_continuation(hip, engine):
    from thinkdiff.models.qwen2_vl import SamplingParams
    prompt = list(range(5, 25))
    forced = torch.randint(0, 4096, (12,), generator=torch.Generator().manual_seed(8)).tolist()
    out = engine.generate(prompt, SamplingParams(max_tokens=12, min_tokens=12, logprobs=0), forced_output_ids=forced)
    assert out["token_ids"] == forced and len(out["logprobs"]) == 12
    ref = _step_logits(engine, prompt, forced)
    want = sum(float(r[t]) for r, t in zip(ref, forced))
    print(f"forced: cumulative_logprob {out['cumulative_logprob']:.6f} vs torch {want:.6f}")
    assert abs(out["cumulative_logprob"] - want) <= 12 * BAR
    for d, t, r in zip(out["logprobs"], forced, ref):
        assert list(d) == [t] and d[t].rank == int((r >= r[t]).sum()) and abs(d[t].logprob - float(r[t])) <= BAR
