"""Per-request LoRA on the Qwen2-VL decode engine, everything that needs no GPU: the C ABI's refusals, the kernel bound held against a float32 restatement
of the kernel, the adapter loader and its refusals, the pool's replacement rule, the prefix-cache salt and the host entries on a stand-in engine."""
import ctypes
import os

import pytest
import torch

import qwen2_lora_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")


def _lib():
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    return lib


def test_abi_version_is_24():
    assert _lib().td_abi_version() >= 24


def _rows_call(lib, x=256, ldx=512, rows=4, K=512, row_adapter=256, n_adapters=1, packed=(256,), ranks=(16,), scales=(1.0,), n_segs=1, y=(256,), ldy=(512,),
               widths=(512,), ws=256, ws_bytes=1 << 30):
    vp = ctypes.c_void_p
    arr = lambda ty, v: (ty * max(1, len(v)))(*v)
    return lib.td_lora_rows_bf16(vp(x), ctypes.c_int64(ldx), rows, K, vp(row_adapter), n_adapters, arr(vp, packed), arr(ctypes.c_int, ranks),
                                 arr(ctypes.c_float, scales), n_segs, arr(vp, y), arr(ctypes.c_int64, ldy), arr(ctypes.c_int, widths), vp(ws),
                                 ctypes.c_size_t(ws_bytes), None)


@pytest.mark.parametrize("kw, word", [
    (dict(x=None), b"null x"),
    (dict(row_adapter=None), b"row_adapter"),
    (dict(ranks=(0,)), b"rank=0"),
    (dict(ranks=(65,)), b"rank=65"),
    (dict(n_adapters=9, packed=(256,) * 9, ranks=(16,) * 9, scales=(1.0,) * 9), b"n_adapters=9"),
    (dict(n_segs=4, y=(256,) * 4, ldy=(512,) * 4, widths=(512,) * 4, packed=(256,) * 4), b"n_segs=4"),
    (dict(n_segs=0), b"n_segs=0"),
    (dict(K=40, ldx=40), b"K=40"),
    (dict(K=0), b"K=0"),
    (dict(widths=(24,)), b"width=24"),
    (dict(y=(None,)), b"null y"),
    (dict(ldy=(500,)), b"ldy=500"),
    (dict(ldx=100), b"ldx=100"),
    (dict(ws=None), b"workspace"),
    (dict(ws_bytes=2000), b"ws_bytes=2000"),
    (dict(scales=(float("inf"),)), b"scale"),
    (dict(rows=0), b"rows=0"),
])
def test_lora_rows_refuses_bad_arguments_before_any_hip_call(kw, word):
    """The pointers are never dereferenced: every refusal is TD_ERR_INVALID and names its argument."""
    lib = _lib()
    rc = _rows_call(lib, **kw)
    assert rc == 2 and word in lib.td_last_error(), (kw, rc, lib.td_last_error())


def test_lora_rows_pack_and_sizes_without_a_gpu():
    lib = _lib()
    one = ctypes.c_void_p(256)
    lib.td_lora_rows_packed_bytes.restype = ctypes.c_size_t
    lib.td_lora_rows_workspace_bytes.restype = ctypes.c_size_t
    assert lib.td_lora_rows_packed_bytes(5, 512, 1536) == (512 + 1536) * 16 * 2
    assert lib.td_lora_rows_packed_bytes(0, 512, 1536) == 0
    # rows padded to 16, the largest r_pad, slabs = min(32, ceil(K / 256)) of equal 32-wide steps: 8960 -> 32, 1536 -> 6
    assert lib.td_lora_rows_workspace_bytes(3, 8960, 3, 64) == 32 * 3 * 16 * 64 * 4
    assert lib.td_lora_rows_workspace_bytes(17, 1536, 1, 5) == 6 * 1 * 32 * 16 * 4
    assert lib.td_lora_rows_workspace_bytes(17, 1500, 1, 5) == 0
    for args, word in (((None, one, 8, 512, 512, one, None), b"null"), ((one, one, 65, 512, 512, one, None), b"rank=65"), ((one, one, 8, 520, 512, one, None), b"N=520"),
                       ((one, one, 8, 512, 100, one, None), b"K=100")):
        rc = lib.td_lora_rows_pack_bf16(*args)
        assert rc == 2 and word in lib.td_last_error(), (args, lib.td_last_error())


def test_engine_lora_entries_refuse_without_a_gpu():
    lib = _lib()
    one = ctypes.c_void_p(256)
    assert lib.td_qwen2_lora_enable(None, 2, 16) == 2 and b"null handle" in lib.td_last_error()
    assert lib.td_qwen2_lora_load(None, 0, b"model.layers.0.mlp.up_proj", one, one, 8, ctypes.c_float(2.0), None) == 2
    assert lib.td_qwen2_lora_remove(None, 0) == 2
    assert lib.td_qwen2_lora_set_slot(None, 0, 0) == 2
    assert lib.td_qwen2_lora_info(None, None, None, None, None) == 2


def test_float32_restatement_meets_the_kernel_bound():
    """The bound the GPU test holds the kernel to, held here against a float32 restatement in another summation order on the same cases: a bound that is too
    tight fails here, without a GPU."""
    worst = 0.0
    for case in C.random_cases():
        for s, base in enumerate(C.case_views(case, case["bufs"])):
            per = [p[s] for p in case["pairs"]]
            y, touched, _ = C.segment_ref(case["x"], base, case["row_adapter"], per, case["scales"])
            bound = C.segment_bound(case["x"], base, case["row_adapter"], per, case["scales"])
            got = C.segment_f32(case["x"], base, case["row_adapter"], per, case["scales"])
            assert torch.equal(got[~touched].view(torch.int16), base[~touched].view(torch.int16))
            if bool(touched.any()):
                ratio = float(((got.double() - y).abs()[touched] / bound[touched]).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (case["layout"], case["x"].shape, s, ratio)
    assert worst > 0.0      # (the two orders do differ somewhere: the check is not vacuous)


def test_exact_cases_are_exact_in_float32():
    """The exact-integer cases of the GPU test: the float32 restatement equals bf16(float64) bit for bit."""
    case = C.make_case("three", 17, 1536, (64, 5), seed=9, exact=True)
    for s, base in enumerate(C.case_views(case, case["bufs"])):
        per = [p[s] for p in case["pairs"]]
        y, touched, ts = C.segment_ref(case["x"], base, case["row_adapter"], per, case["scales"])
        assert all(float(t.abs().max()) <= 256 and torch.equal(t, t.round()) for t in ts.values())
        got = C.segment_f32(case["x"], base, case["row_adapter"], per, case["scales"])
        assert torch.equal(got.double()[touched], y[touched])


# ---- the loader, the pool, the prefix-cache salt and the host entries (no engine, or a stand-in) ---------------------------------------------------------

from oracle import qwen2vl_ref as Q   # noqa: E402

CFG = Q.tiny_config()


def _tc():
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig
    return Qwen2VLTextConfig(hidden_size=CFG.hidden, num_hidden_layers=CFG.num_layers, num_attention_heads=CFG.num_heads, num_key_value_heads=CFG.num_kv_heads,
                             intermediate_size=CFG.intermediate, vocab_size=CFG.vocab)


def _parse(sd, cfg, max_rank=64):
    from thinkdiff.models import qwen2_lora as L
    return L.parse_adapter(sd, cfg, L.module_shapes(_tc()), CFG.num_layers, max_rank)


def _rekey(sd, fn):
    return {fn(k): v for k, v in sd.items()}


def test_loader_maps_every_published_key_spelling():
    sd, cfg = C.make_adapter(CFG, rank=5, seed=1)
    want = _parse(sd, cfg)
    assert want.rank == 5 and want.scale == 2.0 and len(want.pairs) == 7 * CFG.num_layers
    A, B = want.pairs[(1, "mlp.down_proj")]
    assert A.dtype == torch.bfloat16 and torch.equal(A, sd["base_model.model.model.layers.1.mlp.down_proj.lora_A.weight"]) and tuple(B.shape) == (CFG.hidden, 5)
    spellings = [lambda k: k.replace("base_model.model.model.", "base_model.model.model.language_model."),
                 lambda k: k.replace("base_model.model.model.", "base_model.model.language_model.model."),
                 lambda k: k.replace(".lora_A.weight", ".lora_A.default.weight").replace(".lora_B.weight", ".lora_B.default.weight"),
                 lambda k: k[len("base_model.model."):]]
    for fn in spellings:
        got = _parse(_rekey(sd, fn), cfg)
        assert got.pairs.keys() == want.pairs.keys() and all(torch.equal(got.pairs[k][0], want.pairs[k][0]) for k in want.pairs)
    f32 = _parse({k: v.float() * (1 + 2.0 ** -12) for k, v in sd.items()}, cfg)      # another float dtype: rounded to bf16 once, at load
    assert all(torch.equal(f32.pairs[k][1], (want.pairs[k][1].float() * (1 + 2.0 ** -12)).bfloat16()) for k in want.pairs)
    assert _parse(*C.make_adapter(CFG, rank=16, seed=1, use_rslora=True)).scale == 32 / 4      # lora_alpha / sqrt(r)


@pytest.mark.parametrize("change, word", [
    (dict(use_dora=True), "use_dora"), (dict(bias="all"), "bias"), (dict(modules_to_save=["lm_head"]), "modules_to_save"),
    (dict(rank_pattern={"q_proj": 4}), "rank_pattern"), (dict(alpha_pattern={"q_proj": 4}), "alpha_pattern"), (dict(r=128), "max_lora_rank"),
    (dict(peft_type="LOHA"), "peft_type"),
])
def test_loader_refuses_config_fields_by_name(change, word):
    sd, cfg = C.make_adapter(CFG, rank=8, seed=2)
    with pytest.raises(ValueError, match=word):
        _parse(sd, dict(cfg, **change))


def test_loader_refuses_keys_by_name():
    sd, cfg = C.make_adapter(CFG, rank=8, seed=2, modules=("self_attn.q_proj",))
    k0 = "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"
    bad = {
        "lora_embedding_A": {"base_model.model.model.embed_tokens.lora_embedding_A": torch.zeros(8, 4)},
        "embed_tokens": {"base_model.model.model.embed_tokens.lora_A.weight": torch.zeros(8, 4)},
        "lm_head": {"base_model.model.lm_head.lora_A.weight": torch.zeros(8, 4)},
        "visual": {"base_model.model.visual.blocks.0.attn.qkv.lora_A.weight": torch.zeros(8, 4)},
        "layers.7": {"base_model.model.model.layers.7.self_attn.q_proj.lora_A.weight": torch.zeros(8, CFG.hidden)},
        "input_layernorm": {"base_model.model.model.layers.0.input_layernorm.lora_A.weight": torch.zeros(8, CFG.hidden)},
    }
    for word, extra in bad.items():
        with pytest.raises(ValueError, match=word):
            _parse({**sd, **extra}, cfg)
    with pytest.raises(ValueError, match="q_proj.lora_A.weight.*no lora_B"):
        _parse({k: v for k, v in sd.items() if not k.startswith("base_model.model.model.layers.0.self_attn.q_proj.lora_B")}, cfg)
    with pytest.raises(ValueError, match=r"shape \(8, 64\)"):
        _parse({**sd, k0: torch.zeros(8, 64).bfloat16()}, cfg)
    with pytest.raises(ValueError, match="max_lora_rank=4"):
        _parse(sd, cfg, max_rank=4)


def _pool(max_loras=2):
    from thinkdiff.models import qwen2_lora as L
    log = []
    pool = L.LoraPool(max_loras, 16, lambda place, ad: log.append(("load", place, ad.rank)), lambda place: log.append(("remove", place)),
                      lambda slot, place: log.append(("slot", slot, place)))
    for i in (1, 2, 3):
        pool.register(L.LoRARequest(f"ad{i}", i), L.Adapter(i, 2.0, {}))
    return pool, log, [None] + [L.LoRARequest(f"ad{i}", i) for i in (1, 2, 3)]


def test_pool_drops_the_least_recently_used_and_protects_live_adapters():
    pool, log, R = _pool()
    pool.bind([0, 1], [R[1], R[2]])
    assert pool.resident == {1: 0, 2: 1} and ("slot", 0, 0) in log and ("slot", 1, 1) in log
    with pytest.raises(ValueError, match="live sequences"):      # both places are held by live sequences
        pool.bind([2], [R[3]])
    pool.release([0])                                             # adapter 1 is free to go, although adapter 2 was used later
    pool.bind([2], [R[3]])
    assert pool.resident == {2: 1, 3: 0} and log[-3:] == [("remove", 0), ("load", 0, 3), ("slot", 2, 0)] and pool.stats == {"loads": 3, "evictions": 1}
    pool.release_all()
    pool.place([2])                                               # touch 2: now 3 is the least recently used
    pool.bind([0], [R[1]])
    assert sorted(pool.resident) == [1, 2]
    with pytest.raises(ValueError, match="3 distinct LoRA adapters.*max_loras=2"):
        pool.check_call([R[1], R[2], None, R[3]])
    pool.check_call([R[1], R[2], None, R[1]])
    with pytest.raises(ValueError, match="live sequence"):
        pool.forget(1)
    pool.release_all()
    assert pool.forget(1) and not pool.forget(1) and sorted(pool.known) == [2, 3]


def test_vllm_config_keys():
    from thinkdiff.models import qwen2_lora as L
    from thinkdiff.models.qwen2_vl import lora_engine_kwargs_from_vllm_config as kw
    assert kw({}) == {"engine": {}, "lora_request": None} and kw(None)["engine"] == {}
    got = kw({"enable_lora": True, "max_loras": 4, "max_lora_rank": 64, "lora_dtype": "bfloat16", "lora_request": {"lora_name": "x", "lora_int_id": 3, "lora_path": "/p"}})
    assert got == {"engine": {"enable_lora": True, "max_loras": 4, "max_lora_rank": 64}, "lora_request": L.LoRARequest("x", 3, "/p")}
    assert kw({"enable_lora": True})["engine"] == {"enable_lora": True, "max_loras": 1, "max_lora_rank": 16}
    for vc, word in (({"fully_sharded_loras": True}, "fully_sharded_loras"), ({"lora_extra_vocab_size": 256}, "lora_extra_vocab_size"),
                     ({"long_lora_scaling_factors": [4.0]}, "long_lora_scaling_factors"), ({"lora_dtype": "float16"}, "lora_dtype"),
                     ({"enable_lora": True, "max_loras": 9}, "max_loras"), ({"enable_lora": True, "max_lora_rank": 128}, "max_lora_rank"),
                     ({"lora_request": {"lora_name": "x", "lora_int_id": 3}}, "enable_lora"), ({"enable_lora": 1}, "enable_lora"),
                     ({"enable_lora": True, "lora_request": {"lora_name": "x", "lora_int_id": 0}}, "lora_int_id")):
        with pytest.raises(ValueError, match=word):
            kw(vc)


@pytest.mark.parametrize("cls_path", ["thinkdiff.models.mllama_vllm_t5_embed_decoder_2.MllamaVllmT5EmbedDecoderForConditionalGeneration_5",
                                      "thinkdiff.models.mllama_vllm_generate_1.MllamaVllmGenerate_1"])
def test_model_classes_refuse_unserved_lora_keys_before_the_engine_exists(cls_path):
    import importlib
    mod, name = cls_path.rsplit(".", 1)
    cls = getattr(importlib.import_module(mod), name)
    for vc, word in (({"fully_sharded_loras": True}, "fully_sharded_loras"), ({"lora_dtype": "float32"}, "lora_dtype"), ({"lora_extra_vocab_size": 16}, "lora_extra_vocab_size"),
                     ({"long_lora_scaling_factors": [2.0]}, "long_lora_scaling_factors")):
        with pytest.raises(ValueError, match=word):
            cls(_tc(), vllm_config=vc)


def test_block_hashes_are_salted_by_the_adapter():
    from thinkdiff.models import prefix_cache as P
    ids, pos = list(range(40)), Q.text_position_ids(40)
    base = P.block_hashes(ids, pos)
    assert base == P.block_hashes(ids, pos, None, None, None) and len(base) == 2
    a, b = P.block_hashes(ids, pos, adapter=1), P.block_hashes(ids, pos, adapter=2)
    assert a == P.block_hashes(ids, pos, adapter=1) and a != b and a[0] != base[0] and b[1] != base[1]


def test_host_entries_bind_slots_on_a_stand_in_engine(monkeypatch):
    """Slots get their request's adapter before the prefill that fills them, children (n = 2) inherit it, and a freed slot is cleared."""
    import speculative_common as S
    from thinkdiff.models import qwen2_lora as L
    e, Qm, ops = S.fake_engine(n_slots=8, prefill_rows=8)      # (one forward per prompt)
    S.patch(monkeypatch, Qm, ops)
    e.config.num_hidden_layers = 2
    pool = e._lora = L.LoraPool(2, 16, lambda place, ad: e.calls.append(["lora_load", place]), lambda place: e.calls.append(["lora_remove", place]),
                               lambda slot, place: e.calls.append(["lora_slot", slot, place]))
    reqs_l = [L.LoRARequest("x", 5), L.LoRARequest("y", 9)]
    for r in reqs_l:
        pool.register(r, L.Adapter(4, 2.0, {}))
    inherited = []
    monkeypatch.setattr(pool, "inherit", lambda src, dst, orig=pool.inherit: (orig(src, dst), inherited.append((int(src), [int(d) for d in dst], dict(pool.slot_of))))[0])
    reqs = [dict(r, lora_request=l) for r, l in zip(S.prompts(3), [reqs_l[0], None, reqs_l[1]])]
    sps = [Qm.SamplingParams(temperature=1.0, seed=3, n=2, max_tokens=3, min_tokens=3), Qm.SamplingParams(temperature=0.0, max_tokens=2, min_tokens=2),
           Qm.SamplingParams(temperature=0.0, max_tokens=4, min_tokens=4)]
    out = e.generate_batch(reqs, sps)
    assert len(out) == 3 and len(out[0]["outputs"]) == 2
    # every prefilled slot was bound (or known to carry no adapter) before its prefill
    bound = {}
    for c in e.calls:
        if c[0] == "lora_slot":
            bound[c[1]] = c[2]
        elif c[0] == "forward":
            assert (c[1] in bound) == (c[1] in (0, 2)), c
    places = {5: pool.resident[5], 9: pool.resident[9]}
    assert ["lora_slot", 0, places[5]] in e.calls and ["lora_slot", 2, places[9]] in e.calls
    assert inherited and inherited[0][0] == 0 and all(inherited[0][2][d] == 5 for d in inherited[0][1]), "the child of request 0 runs under its adapter"
    assert pool.slot_of == {}, "every slot was released when the call returned"
    cleared = [c[1] for c in e.calls if c[0] == "lora_slot" and c[2] == -1]
    assert 0 in cleared and 2 in cleared and inherited[0][1][0] in cleared
    n_calls = len(e.calls)
    e.generate_batch(S.prompts(2), Qm.SamplingParams(temperature=0.0, max_tokens=2, min_tokens=2))
    assert not [c for c in e.calls[n_calls:] if c[0].startswith("lora_")], "an adapter-less call touches no adapter state"
    with pytest.raises(ValueError, match="3 distinct"):
        pool.register(L.LoRARequest("z", 11), L.Adapter(4, 2.0, {}))
        e.generate_batch([dict(r, lora_request=l) for r, l in zip(S.prompts(3), reqs_l + [L.LoRARequest("z", 11)])], sps[1])
    del e._lora
    with pytest.raises(ValueError, match="enable_lora"):
        e.generate_batch(reqs[:1], sps[1])
