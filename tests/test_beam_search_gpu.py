"""Beam search on the GPU.  td_beam_select against the numpy restatement of its rule (tests/beam_search_common.py) and td_kv_gather_rows against tensor
indexing, both exactly; Qwen2VLTextEngine.beam_search on the tiny decoder of tests/test_parallel_sampling_gpu.py (hidden 512, 2 layers, 4 / 2 heads,
vocab 4096; bf16 and e4m3 cache) against a host-planned loop written here from the pieces the engine had before: decode_batch, logprobs_rows,
fork_slot and host bookkeeping.  Every comparison is an equality."""
import ctypes

import numpy as np
import pytest
import torch

import beam_search_common as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _ops(hip):
    import thinkdiff.ops as ops
    ops.register()      # torch.ops.thinkdiff_hip.*

V = 4096
PROMPTS = [list(range(5, 25)), list(range(40, 57))]


# ---- td_beam_select ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 10])
def test_beam_select_equals_the_restatement(hip, W):
    rng = np.random.default_rng(100 + W)
    seen = {"finisher": 0, "copy": 0, "missing": 0, "tie": 0}
    for R in (1, 3, 16):
        for n_in in sorted({1, W}):
            for cap in (2 * W, 20):
                for _ in range(3):
                    top_ids, top_lp, cum_in, rank_in, eos = C.make_case(rng, R, W, n_in, cap)
                    want = C.select_ref(top_ids, top_lp, cum_in, rank_in, W, n_in, eos)
                    got = hip.beam_select(torch.from_numpy(top_ids).cuda(), torch.from_numpy(top_lp).cuda(), torch.from_numpy(cum_in).cuda(),
                                          torch.from_numpy(rank_in).cuda(), W, n_in, eos)
                    for k, g in zip(C.OUT_KEYS, got):
                        g = g.cpu().numpy()
                        assert not np.isnan(g).any() and np.array_equal(g, want[k]), (k, R, W, n_in, cap, eos, g, want[k])
                    seen["finisher"] += int(want["fin_flag"].sum())
                    seen["copy"] += int((want["copy_src"] >= 0).sum())
                    seen["missing"] += int((want["token"] < 0).sum())
                    live = want["cum_out"][want["token"] >= 0]
                    seen["tie"] += int(len(live) - len(np.unique(live)))
    assert all(v > 0 for k, v in seen.items() if not (W == 1 and k in ("copy", "tie"))), seen


def test_beam_select_writes_log_slices_through_the_op(hip):
    """The op form, writing into slices of [T, R W] logs as the engine does; rows of other steps stay untouched."""
    rng = np.random.default_rng(7)
    R, W, T = 3, 4, 3
    top_ids, top_lp, cum_in, rank_in, eos = C.make_case(rng, R, W, W, 8)
    want = C.select_ref(top_ids, top_lp, cum_in, rank_in, W, W, eos)
    ilog = torch.full((5, T, R * W), -77, dtype=torch.int32, device="cuda")
    flog = torch.full((2, T, R * W), -77.0, dtype=torch.float32, device="cuda")
    torch.ops.thinkdiff_hip.beam_select(torch.from_numpy(top_ids).cuda(), torch.from_numpy(top_lp).cuda(), torch.from_numpy(cum_in).cuda(),
                                        torch.from_numpy(rank_in).cuda(), W, W, eos, ilog[0, 1], flog[0, 1], ilog[1, 1], ilog[2, 1], ilog[3, 1], ilog[4, 1], flog[1, 1])
    for t, k in zip((ilog[0], flog[0], ilog[1], ilog[2], ilog[3], ilog[4], flog[1]), C.OUT_KEYS):
        t = t.cpu().numpy()
        assert np.array_equal(t[1], want[k]) and (t[0] == -77).all() and (t[2] == -77).all(), k


# ---- td_kv_gather_rows ---------------------------------------------------------------------------------------------------------------------------
def _gather_case(hip, row_bytes, slot_rows, n, n_planes, shift, seed, use_op=False):
    """n rows on n + 3 slots in a shuffled order; every third row is a source (copy_src -1) that several later rows copy, some rows copy nothing.
    Each plane lies `shift` bytes into a buffer filled with a canary."""
    g = torch.Generator().manual_seed(seed)
    n_slots = n + 3
    slots = torch.randperm(n_slots, generator=g)[:n].tolist()
    sources = list(range(0, n, 3))
    copy_src = [-1 if (j % 3 == 0 or j % 7 == 5) else sources[(j * 5) % len(sources)] for j in range(n)]
    n_rows = [[0, 1, 7, slot_rows][j % 4] for j in range(n)]
    total = n_slots * slot_rows * row_bytes
    bufs = [torch.full((total + 64,), 0xA5, dtype=torch.uint8) for _ in range(n_planes)]
    for b in bufs:
        b[shift:shift + total] = torch.randint(0, 256, (total,), generator=g, dtype=torch.uint8)
    want = [b.clone() for b in bufs]
    for b, w in zip(bufs, want):
        src_plane, dst_plane = b[shift:shift + total].view(n_slots, slot_rows * row_bytes), w[shift:shift + total].view(n_slots, slot_rows * row_bytes)
        for j, c in enumerate(copy_src):
            if c >= 0:
                dst_plane[slots[j], :n_rows[j] * row_bytes] = src_plane[slots[c], :n_rows[j] * row_bytes]
    dev = [b.cuda() for b in bufs]
    planes = [d[shift:shift + total].view(n_slots * slot_rows, row_bytes) for d in dev]
    src_dev = torch.tensor(copy_src, dtype=torch.int32).cuda()
    if use_op:
        for p in planes:
            torch.ops.thinkdiff_hip.kv_gather_rows(p, slot_rows, slots, src_dev, n_rows)
    else:
        hip.kv_gather_rows([(p, slot_rows) for p in planes], slots, src_dev, n_rows)
    for i, (d, w) in enumerate(zip(dev, want)):
        assert torch.equal(d.cpu(), w), f"plane {i}: row_bytes {row_bytes}, slot_rows {slot_rows}, n {n}, shift {shift}"
    assert sum(1 for c in copy_src if c >= 0) > len(set(c for c in copy_src if c >= 0)), "several destinations share a source"


@pytest.mark.parametrize("row_bytes,slot_rows", [(2, 9), (8, 9), (256, 8), (1024, 8)])
def test_kv_gather_rows_equals_indexing(hip, row_bytes, slot_rows):
    """(2, 9): 2-byte accesses; (8, 9): a 72-byte slot stride, the 8-byte width; 256 and 1024: 16 bytes.  shift 2 leaves every slot 2 bytes off the
    access width, so heads and tails run; n_rows cycles through 0, 1, 7 and slot_rows."""
    for shift in (0, 2):
        _gather_case(hip, row_bytes, slot_rows, n=11, n_planes=2, shift=shift, seed=row_bytes + shift)
    _gather_case(hip, row_bytes, slot_rows, n=6, n_planes=1, shift=0, seed=3, use_op=True)


def test_kv_gather_rows_many_planes_and_rows(hip):
    _gather_case(hip, 8, 9, n=5, n_planes=65, shift=2, seed=1)       # more planes than a launch takes
    _gather_case(hip, 256, 8, n=70, n_planes=1, shift=0, seed=2)     # more rows than a launch's argument block holds
    _gather_case(hip, 16, 8, n=256, n_planes=2, shift=2, seed=4)     # the most a call takes


# ---- the engine ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["auto", "fp8"])
def engine(hip, request):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    return Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                               intermediate_size=1024, vocab_size=V), max_model_len=256, n_slots=8, kv_cache_dtype=request.param).init_random(3, std=0.05)


def _reference(hip, e, prompts, W, T, eos, length_penalty=1.0):
    """The host-planned loop: per step one download of the candidates, the choice on the host, fork_slot for every parent with more than one
    child (into the slots of beams that died), one decode_batch over the beams in rank order.  The prefill is beam_search's: one packed pass into
    slots 0, W, ..  -> per request the W best (tokens, cum, score, finished, hidden rows), and the candidate ids every step saw."""
    R, D = len(prompts), e.config.hidden_size
    plen = [len(p) for p in prompts]
    emb = torch.cat([e.embed_tokens(p) for p in prompts])
    pos = torch.cat([e.text_position_ids(n) for n in plen], dim=1).to(e.device).contiguous()
    hid, logits = torch.empty(sum(plen), D, dtype=torch.bfloat16, device=e.device), torch.empty(R, V, dtype=torch.bfloat16, device=e.device)
    e._prefill_packed_slots(R, (ctypes.c_int * R)(*[r * W for r in range(R)]), emb, pos, (ctypes.c_int * R)(*plen), hid, logits)
    beams = [[{"slot": r * W, "toks": [], "cum": np.float32(0.0), "hid": []}] for r in range(R)]      # per request, in rank order
    completed, seen_ids = [[] for _ in range(R)], []
    for s in range(T):
        n = logits.shape[0]
        _, _, tid, tlp = hip.logprobs_rows(logits, [0] * n, 2 * W, 2 * W)
        tid, tlp = tid.cpu().numpy(), tlp.cpu().numpy()
        seen_ids.append(tid.copy())
        row, feed = 0, []
        for r in range(R):
            cands = []
            for k, b in enumerate(beams[r]):
                for c in range(2 * W):
                    t, cum = int(tid[row, c]), np.float32(b["cum"]) + np.float32(tlp[row, c])
                    if t == eos:
                        completed[r].append((b["toks"] + [t], float(cum), True, list(b["hid"])))
                    else:
                        cands.append((-float(cum), k, c, t, cum))
                row += 1
            cands.sort(key=lambda x: x[:3])
            new, free = [], [sl for sl in range(r * W, r * W + W) if sl not in {beams[r][x[1]]["slot"] for x in cands[:W]}]
            kept = set()
            for _, k, _, t, cum in cands[:W]:
                p = beams[r][k]
                if k in kept:
                    slot = free.pop()
                    e.fork_slot(p["slot"], [slot], plen[r] + s)
                else:
                    kept.add(k)
                    slot = p["slot"]
                new.append({"slot": slot, "toks": p["toks"] + [t], "cum": cum, "hid": list(p["hid"])})
            beams[r] = new
            feed += [(b, plen[r] + s) for b in new]
        h, logits = e.decode_batch([b["toks"][-1] for b, _ in feed], [[n for _, n in feed]] * 3, [n for _, n in feed], slots=[b["slot"] for b, _ in feed])
        for i, (b, _) in enumerate(feed):
            b["hid"].append(h[i])
    out = []
    for r in range(R):
        seqs = completed[r] + [(b["toks"], float(b["cum"]), False, b["hid"]) for b in beams[r]]

        def score(q):
            return q[1] / float(plen[r] + len(q[0]) - (1 if q[0][-1] == eos else 0)) ** float(length_penalty)
        out.append([(q[0], q[1], score(q), q[2], q[3]) for q in sorted(seqs, key=lambda q: -score(q))[:W]])
    return out, seen_ids


def _same(out, want, D=512):
    for o, w in zip(out, want):
        assert len(o["outputs"]) == len(w)
        for c, (toks, cum, score, fin, hid) in zip(o["outputs"], w):
            assert (c["token_ids"], c["cumulative_logprob"], c["score"], c["finished"]) == (toks, cum, score, fin)
            h = torch.stack(hid) if hid else torch.empty(0, D, dtype=torch.bfloat16, device=c["hidden_states"].device)
            assert c["hidden_states"].shape == h.shape and torch.equal(c["hidden_states"], h)
        assert o["token_ids"] == o["outputs"][0]["token_ids"] and torch.equal(o["hidden_states"], o["outputs"][0]["hidden_states"])


@pytest.fixture(scope="module")
def plain(hip, engine):
    """W = 3, T = 6 without an EOS: the reference loop's result and the candidates it saw."""
    return _reference(hip, engine, PROMPTS, 3, 6, eos=-1)


def test_beam_search_equals_the_host_planned_loop(hip, engine, plain):
    from thinkdiff.models.qwen2_vl import BeamSearchParams
    out = engine.beam_search([{"prompt_token_ids": p} for p in PROMPTS], BeamSearchParams(beam_width=3, max_tokens=6))
    want, _ = plain
    _same(out, want)
    for o, p in zip(out, PROMPTS):
        assert o["prompt_hidden_states"].shape == (len(p), 512) and all(len(c["token_ids"]) == 6 and not c["finished"] for c in o["outputs"])
        assert [c["cumulative_logprob"] for c in o["outputs"]] == sorted((c["cumulative_logprob"] for c in o["outputs"]), reverse=True)
        assert len({tuple(c["token_ids"]) for c in o["outputs"]}) == 3


@pytest.mark.parametrize("length_penalty", [1.0, 0.0])
def test_beam_search_with_an_eos_among_the_candidates(hip, engine, plain, length_penalty):
    """EOS = the second candidate of request 0's best beam at the third step: from there on a completed sequence exists and the search differs."""
    from thinkdiff.models.qwen2_vl import BeamSearchParams
    _, seen = plain
    eos = int(seen[2][0, 1])
    want, _ = _reference(hip, engine, PROMPTS, 3, 6, eos=eos, length_penalty=length_penalty)
    out = engine.beam_search([{"prompt_token_ids": p} for p in PROMPTS], BeamSearchParams(beam_width=3, max_tokens=6, length_penalty=length_penalty), eos_token_id=eos)
    _same(out, want)
    again = engine.beam_search([{"prompt_token_ids": p} for p in PROMPTS], BeamSearchParams(beam_width=3, max_tokens=6, length_penalty=length_penalty, ignore_eos=True),
                               eos_token_id=eos)
    assert not any(c["finished"] for o in again for c in o["outputs"])
    if length_penalty == 0.0:      # scores are the cumulative logprobs: a sequence completed at step 3 with the best beam's second candidate is among the best
        assert any(c["finished"] and c["token_ids"][-1] == eos for c in out[0]["outputs"]), [c["token_ids"] for c in out[0]["outputs"]]


def test_width_one_is_greedy_decoding(hip, engine):
    from thinkdiff.models.qwen2_vl import BeamSearchParams, SamplingParams
    g = engine.generate(PROMPTS[0], SamplingParams(temperature=0.0, max_tokens=6, min_tokens=6, ignore_eos=True, logprobs=2))
    for d in g["logprobs"]:
        top = sorted((v.logprob for v in d.values()), reverse=True)
        assert top[0] > top[1], "the top two logits of a step tie: greedy decoding is not defined by the values alone"
    o = engine.beam_search([{"prompt_token_ids": PROMPTS[0]}], BeamSearchParams(beam_width=1, max_tokens=6, ignore_eos=True))[0]
    assert o["token_ids"] == g["token_ids"] and len(o["outputs"]) == 1 and o["hidden_states"].shape == (6, 512)
    assert o["cumulative_logprob"] == pytest.approx(g["cumulative_logprob"], rel=1e-5)


def test_gather_slots_moves_cache_rows(hip, engine):
    from thinkdiff.models.qwen2_vl import SamplingParams
    reqs = [{"prompt_token_ids": PROMPTS[0]}, {"prompt_token_ids": PROMPTS[1]}, {"prompt_token_ids": PROMPTS[0][:9]}]
    engine.generate_batch(reqs, SamplingParams(temperature=0.0, max_tokens=2, min_tokens=2))      # slots 0, 1, 2 hold 22, 19 and 11 rows
    def bits(l, s):      # (compared as bits: rows nobody wrote yet may hold anything, NaN included)
        return engine.read_kv(l, s, 0, 32).view(torch.int16).clone()
    before = {(l, s): bits(l, s) for l in range(2) for s in range(8)}
    # rows: slot 5 <- slot 0 (22 rows), slot 1 stays, slot 6 <- slot 2 (11 rows), slot 0 and 2 are sources, slot 7 <- slot 0 (5 rows), slot 3 names itself
    slots, src, lens = [5, 1, 6, 0, 2, 7, 3], [3, -1, 4, -1, -1, 3, 6], [22, 19, 11, 22, 11, 5, 9]
    engine.gather_slots(slots, torch.tensor(src, dtype=torch.int32).cuda(), lens)
    for l in range(2):
        after = {s: bits(l, s) for s in range(8)}
        for dst, s0, n in [(5, 0, 22), (6, 2, 11), (7, 0, 5)]:
            assert torch.equal(after[dst][:n], before[(l, s0)][:n]) and torch.equal(after[dst][n:], before[(l, dst)][n:]), (l, dst)
        for s in (0, 1, 2, 3, 4):
            assert torch.equal(after[s], before[(l, s)]), (l, s)
    with pytest.raises(hip.ThinkDiffHipError, match="slot 8 of row 1 outside the 8 configured sequences"):
        engine.gather_slots([0, 8], torch.tensor([-1, -1], dtype=torch.int32).cuda(), [1, 1])
    with pytest.raises(hip.ThinkDiffHipError, match="len=257 of row 0 exceeds the slot capacity 256"):
        engine.gather_slots([0, 1], torch.tensor([-1, -1], dtype=torch.int32).cuda(), [257, 1])
