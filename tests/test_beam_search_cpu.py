"""Beam search without a GPU: BeamSearchParams and its refusals, the argument errors of td_beam_select / td_kv_gather_rows / td_qwen2_gather_slots,
the op schemas, the vllm_config keys on both model classes, properties of the select rule's restatement (tests/beam_search_common.py) and the host
logic of Qwen2VLTextEngine.beam_search on the stand-in engine against an independent brute-force beam search."""
import ctypes
import importlib
import itertools
import os

import numpy as np
import pytest
import torch

import beam_search_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")


def test_validate_refusals():
    from thinkdiff.models.qwen2_vl import BeamSearchParams
    ok = BeamSearchParams(beam_width=4, max_tokens=8).validate()
    assert (ok.ignore_eos, ok.temperature, ok.length_penalty) == (False, 0.0, 1.0)
    assert BeamSearchParams(beam_width=10, max_tokens=1, temperature=0, length_penalty=0).validate().beam_width == 10
    for kw, field in [(dict(beam_width=0), "beam_width"), (dict(beam_width=11), "beam_width"), (dict(beam_width=2.0), "beam_width"), (dict(beam_width=True), "beam_width"),
                      (dict(beam_width="4"), "beam_width"), (dict(beam_width=None), "beam_width"), (dict(max_tokens=0), "max_tokens"), (dict(max_tokens=1.5), "max_tokens"),
                      (dict(max_tokens=None), "max_tokens"), (dict(temperature=0.6), "temperature"), (dict(temperature=None), "temperature"),
                      (dict(temperature=float("nan")), "temperature"), (dict(length_penalty=float("inf")), "length_penalty"),
                      (dict(length_penalty=float("nan")), "length_penalty"), (dict(length_penalty="1"), "length_penalty"), (dict(ignore_eos=1), "ignore_eos")]:
        with pytest.raises(ValueError, match=rf"BeamSearchParams\.{field}="):
            BeamSearchParams(**{**dict(beam_width=2, max_tokens=4), **kw}).validate()


# ---- C ABI without a GPU -------------------------------------------------------------------------------------------------------------------------
class _Plane(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("row_bytes", ctypes.c_int64), ("slot_rows", ctypes.c_int64)]


def _lib():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    return lib


def test_abi_version():
    assert _lib().td_abi_version() >= 18


def test_beam_select_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.td_beam_select.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    names = ["top_ids", "top_lp", "cum_in", "rank_in", "token", "cum_out", "rank_out", "copy_src", "parent", "fin_flag", "fin_cum"]

    def call(null=None, cap=8, R=2, W=4, n_in=4, eos=-1):
        p = {k: (None if k == null else 256) for k in names}      # (never dereferenced: every refusal comes before any HIP call)
        rc = lib.td_beam_select(p["top_ids"], p["top_lp"], cap, p["cum_in"], p["rank_in"], R, W, n_in, eos, p["token"], p["cum_out"], p["rank_out"], p["copy_src"],
                                p["parent"], p["fin_flag"], p["fin_cum"], None)
        return rc, lib.td_last_error().decode()

    for k in names:
        rc, msg = call(null=k)
        assert rc == 2 and "null" in msg, (k, rc, msg)
    for kw, word in [(dict(W=0, n_in=0), "W=0"), (dict(W=11, n_in=11, cap=22), "W=11"), (dict(cap=7), "cap=7"), (dict(n_in=2), "n_in=2"), (dict(n_in=0), "n_in=0"),
                     (dict(R=0), "R=0"), (dict(R=-3), "R=-3"), (dict(R=16384), "R*W=65536")]:
        rc, msg = call(**kw)
        assert rc == 2 and word in msg, (kw, rc, msg)


def test_kv_gather_rows_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.td_kv_gather_rows.argtypes = [vp, i32, i32, vp, vp, vp, vp]

    def call(planes=((256, 512, 64),), slots=(0, 1, 2), n_rows=(8, 8, 8), n=None, n_planes=None, null=None):
        arr = (_Plane * max(1, len(planes)))(*[_Plane(*p) for p in planes])
        sl, nr = (i32 * max(1, len(slots)))(*slots), (i32 * max(1, len(n_rows)))(*n_rows)
        rc = lib.td_kv_gather_rows(None if null == "planes" else ctypes.cast(arr, vp), len(planes) if n_planes is None else n_planes, len(slots) if n is None else n,
                                   None if null == "slots" else ctypes.cast(sl, vp), None if null == "copy_src_dev" else 256,
                                   None if null == "n_rows" else ctypes.cast(nr, vp), None)
        return rc, lib.td_last_error().decode()

    for kw, word in [(dict(null="planes"), "null planes"), (dict(null="slots"), "null slots"), (dict(null="copy_src_dev"), "null copy_src_dev"),
                     (dict(null="n_rows"), "null n_rows"), (dict(n_planes=0), "n_planes=0"), (dict(n=0), "n=0"), (dict(n=257), "n=257"),
                     (dict(slots=(0, -2, 1)), "slot -2"), (dict(slots=(3, 1, 3)), "slot 3 is given twice"), (dict(n_rows=(8, -1, 8)), "n_rows=-1"),
                     (dict(n_rows=(8, 65, 8)), "n_rows=65"), (dict(planes=((256, 512, 64), (256, 8, 5)), n_rows=(6, 0, 0)), "slot_rows=5 of plane 1"),
                     (dict(planes=((256, 7, 64),)), "row_bytes=7"), (dict(planes=((256, 0, 64),)), "row_bytes=0"), (dict(planes=((0, 8, 64),)), "null base"),
                     (dict(planes=((257, 8, 64),)), "not 2-byte aligned")]:
        rc, msg = call(**kw)
        assert rc == 2 and word in msg, (kw, rc, msg)
    assert call(n_rows=(0, 0, 0))[0] == 0, "no rows: TD_OK and no launch"
    lib.td_qwen2_gather_slots.argtypes = [vp, i32, vp, vp, vp, vp]
    one = ctypes.cast((i32 * 1)(0), vp)
    assert lib.td_qwen2_gather_slots(None, 1, one, 256, one, None) == 2 and b"null handle" in lib.td_last_error()


def test_op_schemas_and_bindings():
    import thinkdiff.ops as ops
    from thinkdiff import _hip
    ops.register()
    assert ops.SCHEMAS["kv_gather_rows"] == "(Tensor(a!) plane, int slot_rows, int[] slots, Tensor copy_src, int[] n_rows) -> ()"
    assert ops.SCHEMAS["beam_select"].startswith("(Tensor top_ids, Tensor top_lp, Tensor cum_in, Tensor rank_in, int W, int n_in, int eos, Tensor(a!) token, ")
    for name in ("kv_gather_rows", "beam_select"):
        assert str(getattr(torch.ops.thinkdiff_hip, name).default._schema) == f"thinkdiff_hip::{name}{ops.SCHEMAS[name]}"
    with pytest.raises((NotImplementedError, RuntimeError)):      # no host kernel to fall back to
        torch.ops.thinkdiff_hip.kv_gather_rows(torch.zeros(8, 16, dtype=torch.uint8), 4, [0, 1], torch.tensor([-1, 0], dtype=torch.int32), [2, 2])
    i, f = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float32)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.thinkdiff_hip.beam_select(torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4), f, i, 2, 2, -1, i.clone(), f.clone(), i.clone(), i.clone(), i.clone(),
                                            i.clone(), f.clone())
    assert _hip.MAX_BEAM_WIDTH == 10 and 2 * _hip.MAX_BEAM_WIDTH <= _hip.MAX_LOGPROBS and callable(_hip.beam_select) and callable(_hip.kv_gather_rows)
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine
    assert callable(Qwen2VLTextEngine.gather_slots) and callable(Qwen2VLTextEngine.beam_search)


# ---- vllm_config ---------------------------------------------------------------------------------------------------------------------------------
def test_beam_params_from_vllm_config():
    from thinkdiff.models import qwen2_vl as Q
    assert Q.BEAM_CONFIG_KEYS == ("beam_width", "length_penalty")
    assert Q.PARALLEL_CONFIG_KEYS == ("n", "best_of") and "beam_width" not in Q.sampler_fields_from_vllm_config({"beam_width": 4, "seed": 1})
    assert Q.beam_params_from_vllm_config({"max_tokens": 9}) is None and Q.beam_params_from_vllm_config({"beam_width": None}) is None
    bp = Q.beam_params_from_vllm_config({"beam_width": 4}, max_tokens=77, ignore_eos=True)
    assert (bp.beam_width, bp.max_tokens, bp.ignore_eos, bp.temperature, bp.length_penalty) == (4, 77, True, 0.0, 1.0)
    bp = Q.beam_params_from_vllm_config({"beam_width": 3, "length_penalty": 0.5, "max_tokens": 5, "ignore_eos": False, "temperature": 0.0, "n": 1}, max_tokens=77, ignore_eos=True)
    assert (bp.beam_width, bp.max_tokens, bp.ignore_eos, bp.length_penalty) == (3, 5, False, 0.5)
    for vc, word in [({"beam_width": 4, "n": 2}, "together with"), ({"beam_width": 4, "best_of": 3}, "together with"), ({"beam_width": 11}, r"BeamSearchParams\.beam_width=11"),
                     ({"beam_width": 4, "temperature": 0.6}, r"BeamSearchParams\.temperature=0.6"), ({"length_penalty": 2.0}, "without beam_width")]:
        with pytest.raises(ValueError, match=word):
            Q.beam_params_from_vllm_config(vc)


@pytest.mark.parametrize("cls_path", ["thinkdiff.models.mllama_vllm_t5_embed_decoder_2:MllamaVllmT5EmbedDecoderForConditionalGeneration_5",
                                      "thinkdiff.models.mllama_vllm_generate_1:MllamaVllmGenerate_1"])
def test_beam_width_routes_the_model_classes_through_beam_search(cls_path, monkeypatch):
    mod_name, name = cls_path.split(":")
    mod = importlib.import_module(mod_name)
    seen = []

    class Engine(mod.Qwen2VLTextEngine):      # no HIP handle
        def __init__(self, *a, **kw):
            pass

        def __del__(self):
            pass

        def beam_search(self, requests, params, eos_token_id=None):
            seen.append((len(requests), params, eos_token_id))
            return [{"prompt_hidden_states": torch.zeros(len(r["prompt_token_ids"]), 4), "hidden_states": torch.ones(2, 4), "token_ids": [5, 6],
                     "outputs": [{"index": 0}]} for r in requests]

        def generate_batch(self, *a, **kw):
            raise AssertionError("beam_width set: generation goes through beam_search")

        generate = generate_continuous = generate_batch

    monkeypatch.setattr(mod, "Qwen2VLTextEngine", Engine)
    if hasattr(mod, "HipVisionProjector"):
        monkeypatch.setattr(mod, "HipVisionProjector", lambda *a, **kw: (lambda x: x))
    cls = getattr(mod, name)
    assert cls(vllm_config={"max_model_len": 64}).mllama_beam_params is None
    vc = {"max_model_len": 64, "beam_width": 4, "max_num_seqs": 8, "max_tokens": 6, "length_penalty": 2.0, "eos_token_id": 9, "ignore_eos": False}
    for bad, word in [({"n": 2}, "together with"), ({"best_of": 2}, "together with"), ({"temperature": 0.7}, r"BeamSearchParams\.temperature"), ({"beam_width": 0}, "beam_width=0")]:
        with pytest.raises(ValueError, match=word):
            cls(vllm_config={**vc, **bad})
    prompts = [[1, 2, 3], [4, 5], [6], [7, 8], [9, 10, 11]]
    if name == "MllamaVllmGenerate_1":
        monkeypatch.setenv("TD_PRECOMPUTE_PREFETCH", "0")      # (the helper thread builds requests on a GPU stream)
        m = cls(vllm_config=vc, request_builder=lambda samples, i: {"prompt_token_ids": samples["answers"][i]})
        out = m.forward_inner({"answers": prompts})
        assert out["generated_token"]["output_token_ids"] == [(5, 6)] * 5
    else:
        m = cls(vllm_config=vc)
        monkeypatch.setattr(m, "resolve_requests", lambda reqs: reqs)
        reqs = [{"prompt_token_ids": p} for p in prompts]
        emb, texts = m.get_embed(reqs, embedding_type="output_embed", need_process=False)
        assert texts == ["5 6"] * 5 and all(torch.equal(x, torch.ones(2, 4)) for x in emb)
        with pytest.raises(ValueError, match="forced_output_ids"):
            m.get_embed(reqs, need_process=False, forced_output_ids=[[1]] * 5)
    bp = m.mllama_beam_params
    assert (bp.beam_width, bp.max_tokens, bp.length_penalty, bp.ignore_eos) == (4, 6, 2.0, False)
    assert [n for n, _, _ in seen] == [2, 2, 1], "chunks of max_num_seqs // beam_width requests"
    assert all(p is bp and eos == 9 for _, p, eos in seen)


# ---- the rule's restatement ----------------------------------------------------------------------------------------------------------------------
def _random_case(rng):
    W, R = int(rng.integers(1, 11)), int(rng.integers(1, 4))
    n_in = 1 if rng.random() < 0.25 else W
    top_ids, top_lp, cum_in, rank_in, eos = C.make_case(rng, R, W, n_in, 2 * W if rng.random() < 0.5 else 20)
    return top_ids, top_lp, cum_in, rank_in, W, n_in, eos


def test_restatement_properties_over_random_cases():
    rng = np.random.default_rng(11)
    copies = 0
    for _ in range(1000):
        top_ids, top_lp, cum_in, rank_in, W, n_in, eos = _random_case(rng)
        o = C.select_ref(top_ids, top_lp, cum_in, rank_in, W, n_in, eos)
        N = len(cum_in)
        assert not np.isnan(o["cum_out"]).any() and not np.isnan(o["fin_cum"]).any()
        for base in range(0, N, W):
            rows = np.arange(base, base + W)
            src = {int(s) for s in o["copy_src"][rows] if s >= 0}
            dst = {int(r) for r in rows if o["copy_src"][r] >= 0}
            copies += len(dst)
            assert not src & dst, "a row is both read and written"
            assert all(base <= s < base + min(n_in, W) for s in src), "a source is a live row of the same request"
            for s in src:
                assert o["parent"][s] == s and o["token"][s] >= 0, "a source row keeps its own beam"
            assert sorted(o["rank_out"][rows].tolist()) == list(range(W)), "ranks are a permutation"
            for r in rows:
                assert o["parent"][r] == (o["copy_src"][r] if o["copy_src"][r] >= 0 else r)
            # a plain sort of the same candidates: the beams in rank order are its first W
            flat = []
            for j in range(n_in):
                for c in range(2 * W):
                    t = int(top_ids[base + j, c])
                    if t >= 0 and not (eos >= 0 and t == eos):
                        flat.append((-float(np.float32(cum_in[base + j]) + np.float32(top_lp[base + j, c])), int(rank_in[base + j]), c, t, base + j))
            flat.sort()
            by_rank = sorted(rows, key=lambda r: o["rank_out"][r])
            got = [(int(o["token"][r]), float(o["cum_out"][r]), int(o["parent"][r])) for r in by_rank]
            want = [(t, -negcum, row) for negcum, _, _, t, row in flat[:W]]
            assert got[:len(want)] == want
            assert all(g[0] == -1 and g[1] == -np.inf for g in got[len(want):]), "missing beams: token -1, cum -inf"
            for j in range(W):
                hit = [c for c in range(2 * W) if j < n_in and eos >= 0 and top_ids[base + j, c] == eos]
                assert o["fin_flag"][base + j] == (1 if hit else 0)
                if hit:
                    assert o["fin_cum"][base + j] == np.float32(cum_in[base + j]) + np.float32(top_lp[base + j, hit[0]])
    assert copies > 1000, "the cases exercise the placement"


# ---- the host logic on the stand-in ---------------------------------------------------------------------------------------------------------------
PROMPTS = [[3, 1, 4, 1, 5], [9, 2, 6]]


def _eos_that_occurs(prompt, W, T, length_penalty=1.0):
    """A token that completes a sequence in some round without ending the search: the brute force tells.  One whose completed sequence is among the
    W returned is preferred."""
    some = [eos for eos in range(C.V) if any(f for *_, f in C.brute_force(prompt, W, T, eos, False, length_penalty, keep_all=True))]
    shown = [eos for eos in some if any(f for *_, f in C.brute_force(prompt, W, T, eos, False, length_penalty))]
    assert some
    return (shown or some)[0]


@pytest.mark.parametrize("W,with_eos,length_penalty", list(itertools.product([1, 2, 3], [False, True], [0.0, 1.0, 2.0])))
def test_beam_search_on_the_stand_in_equals_the_brute_force(W, with_eos, length_penalty, monkeypatch):
    T = 4
    e, Q, ops = C.fake_engine(n_slots=2 * W)
    C.patch(monkeypatch, e, Q, ops)
    eos = _eos_that_occurs(PROMPTS[0], W, T, length_penalty) if with_eos else None
    reqs = [{"prompt_token_ids": p} for p in PROMPTS]
    out = e.beam_search(reqs, Q.BeamSearchParams(beam_width=W, max_tokens=T, length_penalty=length_penalty), eos_token_id=eos)
    assert e.loop_downloads == 0 and e.downloads > e.in_loop, "no download between the loop's first op and its last decode step; the logs are read afterwards"
    assert [c[0] for c in e.calls if c[0] in ("prefill", "forward")] == ["prefill"] and e.calls[0][1] == [0, W], "one packed prefill, request r into slot r W"
    loop = [c[0] for c in e.calls[1:]]
    assert loop == ["logprobs_rows", "beam_select", "gather", "decode"] * T
    assert [c[2] for c in e.calls if c[0] == "beam_select"] == [1] + [W] * (T - 1) and all(c[3] == (-1 if eos is None else eos) for c in e.calls if c[0] == "beam_select")
    with e.own():
        for r, (p, o) in enumerate(zip(PROMPTS, out)):
            want = C.brute_force(p, W, T, eos, False, length_penalty)
            outs = o["outputs"]
            assert len(outs) == W and [c["index"] for c in outs] == list(range(W))
            assert [(c["token_ids"], c["cumulative_logprob"], c["score"], c["finished"]) for c in outs] == want
            assert o["token_ids"] == outs[0]["token_ids"] and torch.equal(o["hidden_states"], outs[0]["hidden_states"])
            assert (o["cumulative_logprob"], o["score"]) == (outs[0]["cumulative_logprob"], outs[0]["score"])
            assert o["prompt_hidden_states"][:, 0].float().tolist() == [float(t) for t in p]
            for c in outs:
                fed = c["token_ids"][:-1] if c["finished"] else c["token_ids"]      # the EOS of a completed sequence is never fed
                h = c["hidden_states"].float()
                assert h.shape == (len(fed), C.D) and h[:, 0].tolist() == [float(t) for t in fed]
                assert h[:, 2].tolist() == [float(s) for s in range(len(fed))] and h[:, 3].tolist() == [float(len(p) + s) for s in range(len(fed))]
                for s in range(len(fed)):      # the row named at step s held exactly this beam's ancestor
                    row = int(h[s, 1])
                    assert r * W <= row < (r + 1) * W and e.held[s][row] == p + fed[:s + 1]
        if with_eos:
            assert any(c["finished"] for c in out[0]["outputs"]), "the chosen EOS completes a sequence of request 0"


def test_ignore_eos_and_a_single_request(monkeypatch):
    e, Q, ops = C.fake_engine(n_slots=3)
    C.patch(monkeypatch, e, Q, ops)
    eos = _eos_that_occurs(PROMPTS[0], 3, 4)
    out = e.beam_search([{"prompt_token_ids": PROMPTS[0]}], Q.BeamSearchParams(beam_width=3, max_tokens=4, ignore_eos=True, length_penalty=2.0), eos_token_id=eos)
    assert e.calls[0] == ["forward", 0, 5] and all(c[3] == -1 for c in e.calls if c[0] == "beam_select"), "one prompt: a forward; ignore_eos: the kernel sees no EOS"
    want = C.brute_force(PROMPTS[0], 3, 4, eos, True, 2.0)
    with e.own():
        assert [(c["token_ids"], c["cumulative_logprob"], c["score"], c["finished"]) for c in out[0]["outputs"]] == want
    assert not any(f for _, _, _, f in want)


def test_beam_search_refusals_come_before_anything_runs(monkeypatch):
    from thinkdiff import _hip
    e, Q, ops = C.fake_engine(n_slots=6, slot_len=10)
    C.patch(monkeypatch, e, Q, ops)
    reqs = [{"prompt_token_ids": p} for p in PROMPTS]
    bp = Q.BeamSearchParams
    with pytest.raises(_hip.ThinkDiffHipError, match=r"2 requests x beam_width=4 need 8 cache slots, which exceed min\(256, n_slots=6\)"):
        e.beam_search(reqs, bp(beam_width=4, max_tokens=2))
    with pytest.raises(_hip.ThinkDiffHipError, match=r"request 0: prompt length 5 \+ max_tokens=6 exceeds the slot capacity 10"):
        e.beam_search(reqs, bp(beam_width=2, max_tokens=6))
    with pytest.raises(ValueError, match=r"vocab_size=12 must exceed 2 x beam_width = 12"):
        e.beam_search(reqs[:1], bp(beam_width=6, max_tokens=2))
    with pytest.raises(ValueError, match=r"BeamSearchParams\.temperature=0.5"):
        e.beam_search(reqs, bp(beam_width=2, max_tokens=2, temperature=0.5))
    with pytest.raises(ValueError, match="eos_token_id=12"):
        e.beam_search(reqs, bp(beam_width=2, max_tokens=2), eos_token_id=12)
    with pytest.raises(ValueError, match="no requests"):
        e.beam_search([], bp(beam_width=2, max_tokens=2))
    assert e.calls == []
