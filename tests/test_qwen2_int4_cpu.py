"""The grouped int4 (AWQ / GPTQ) weight stream of the Qwen2-VL decode engine without a GPU: the exported / declared / bound symbols and the ABI version, the
C ABI's argument errors (TD_ERR_INVALID with a message, before any HIP call), the CPU restatement's checkpoint packers (tests/qwen2_int4_common.py), every
refusal of the checkpoint loader by key or field, `quantization_config` detection, and the unchanged `quantization` keyword."""
import ctypes
import json
import os
import re
import types

import pytest
import torch

import qwen2_int4_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
HEADER = os.path.join(ROOT, "include", "thinkdiff_hip.h")
TD_ERR_INVALID = 2

SYMBOLS = ["td_repack_int4", "td_dequant_rows_int4", "td_linear_i4_bf16", "td_linear_split_i4_bf16", "td_linear_glu_i4_bf16", "td_qwen2_load_param_int4",
           "td_qwen2_set_int4_routing"]


# ---- symbols and ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound():
    lib = ctypes.CDLL(LIB)
    header = open(HEADER).read()
    from thinkdiff import _hip
    sig = _hip._declare(lib)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/thinkdiff_hip.h"
        assert name in sig, f"{name} is not bound in thinkdiff/_hip.py"
    assert re.search(r"TD_QWEN2_WEIGHTS_INT4\s*=\s*3", header) and _hip.QWEN2_WEIGHTS_INT4 == 3
    assert re.search(r"TD_INT4_AWQ\s*=\s*0", header) and re.search(r"TD_INT4_GPTQ\s*=\s*1", header) and re.search(r"TD_INT4_GPTQ_V2\s*=\s*2", header)
    assert (_hip.INT4_AWQ, _hip.INT4_GPTQ, _hip.INT4_GPTQ | _hip.INT4_GPTQ_V2) == (C.LAYOUT_AWQ, C.LAYOUT_GPTQ, C.LAYOUT_GPTQ_V2)
    assert lib.td_abi_version() >= 22
    for fn in ("repack_int4", "dequant_rows_int4", "linear_i4", "linear_split_i4", "linear_glu_i4"):
        assert callable(getattr(_hip, fn))
    from thinkdiff import ops
    for op in ("repack_int4", "dequant_rows_int4", "linear_i4"):
        assert op in ops.SCHEMAS and hasattr(torch.ops.thinkdiff_hip, op)


def _lib():
    from thinkdiff import _hip
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    _hip._declare(lib)
    return lib


def _buf(nbytes, offset=0):
    """A 64-byte aligned host buffer (+ offset): the entries under test refuse before anything would read it."""
    raw = ctypes.create_string_buffer(nbytes + 128)
    base = (ctypes.addressof(raw) + 63) & ~63
    return raw, ctypes.c_void_p(base + offset)


def test_linear_i4_argument_errors_come_before_any_hip_call():
    lib = _lib()
    keep, x = _buf(1 << 16)
    keep2, wq = _buf(1 << 16)
    keep3, sc = _buf(1 << 12)
    keep4, zp = _buf(1 << 12)
    keep5, y = _buf(1 << 16)
    keep6, x_odd = _buf(1 << 16, offset=2)
    keep7, wq_odd = _buf(1 << 16, offset=8)
    keep8, sc_odd = _buf(1 << 12, offset=4)
    keep9, zp_odd = _buf(1 << 12, offset=4)

    def call(x=x, ldx=256, wq=wq, sc=sc, zp=zp, G=128, y=y, ldy=64, M=4, N=64, K=256):
        return lib.td_linear_i4_bf16(x, ldx, wq, sc, zp, G, None, y, ldy, M, N, K, 0, None, None, 0, None), lib.td_last_error().decode()

    rc, msg = call(M=65)
    assert rc == TD_ERR_INVALID and "M=65" in msg and "64" in msg
    for kw in ({"x": None}, {"wq": None}, {"sc": None}, {"zp": None}, {"y": None}):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "required" in msg, (kw, msg)
    for kw in ({"x": x_odd}, {"wq": wq_odd}, {"sc": sc_odd}, {"zp": zp_odd}):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "aligned" in msg, (kw, msg)
    for G in (0, 16, 48, 256, -128):
        rc, msg = call(G=G)
        assert rc == TD_ERR_INVALID and f"G={G}" in msg and "32, 64 and 128" in msg
    rc, msg = call(K=100, ldx=104, G=32)       # K % 32 != 0: not a whole number of 16-byte chunks
    assert rc == TD_ERR_INVALID and "K=100" in msg
    rc, msg = call(K=192, ldx=192, G=128)      # K % G != 0
    assert rc == TD_ERR_INVALID and "K=192" in msg and "G=128" in msg
    rc, msg = call(M=17, K=384, ldx=384)       # more than 16 rows need the matrix-core form: K % 256 == 0
    assert rc == TD_ERR_INVALID and "K=384" in msg and "256" in msg
    rc, msg = call(N=62)
    assert rc == TD_ERR_INVALID and "N=62" in msg
    rc, msg = call(ldx=128)
    assert rc == TD_ERR_INVALID and "lda=128" in msg
    assert call(M=0)[0] == TD_ERR_INVALID
    # the split and gated entries share the checks
    rc = lib.td_linear_split_i4_bf16(x, 256, wq, sc, zp, 128, None, y, 64, 0, None, 64, 0, 4, 64, 256, 32, None)
    assert rc == TD_ERR_INVALID and "y1" in lib.td_last_error().decode()
    rc = lib.td_linear_split_i4_bf16(x, 256, wq, sc, zp, 128, None, y, 64, 0, y, 64, 0, 4, 64, 256, 30, None)
    assert rc == TD_ERR_INVALID and "split" in lib.td_last_error().decode()
    rc = lib.td_linear_split_i4_bf16(x, 256, wq, sc, zp, 96, None, y, 64, 0, y, 64, 0, 4, 64, 256, 32, None)
    assert rc == TD_ERR_INVALID and "G=96" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_i4_bf16(x, 256, wq, sc, zp, 128, y, 64, 65, 64, 256, None)
    assert rc == TD_ERR_INVALID and "M=65" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_i4_bf16(x, 256, wq, sc, zp, 128, y, 64, 4, 60, 256, None)
    assert rc == TD_ERR_INVALID and "glu" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_i4_bf16(x, 256, wq, sc, None, 128, y, 64, 4, 64, 256, None)
    assert rc == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_i4_bf16(x, 256, wq, sc, zp, 7, y, 64, 4, 64, 256, None)
    assert rc == TD_ERR_INVALID and "G=7" in lib.td_last_error().decode()


def test_repack_and_dequant_argument_errors_come_before_any_hip_call():
    lib = _lib()
    keep, qw = _buf(1 << 16)
    keep2, qz = _buf(1 << 12)
    keep3, sc = _buf(1 << 14)
    keep4, pk = _buf(1 << 16)
    keep5, so = _buf(1 << 14)
    keep6, zo = _buf(1 << 12)
    keep7, qw_odd = _buf(1 << 16, offset=2)
    keep8, pk_odd = _buf(1 << 16, offset=2)
    keep9, sc_odd = _buf(1 << 14, offset=1)
    keep10, w = _buf(1 << 16)
    keep11, w_odd = _buf(1 << 16, offset=4)

    def rp(layout=0, qw=qw, qz=qz, sc=sc, N=64, K=256, G=128, pk=pk, so=so, zo=zo):
        return lib.td_repack_int4(layout, qw, qz, sc, None, N, K, G, pk, so, zo, None), lib.td_last_error().decode()

    for kw in ({"qw": None}, {"qz": None}, {"sc": None}, {"pk": None}, {"so": None}, {"zo": None}):
        rc, msg = rp(**kw)
        assert rc == TD_ERR_INVALID and "required" in msg, (kw, msg)
    for kw in ({"qw": qw_odd}, {"pk": pk_odd}, {"sc": sc_odd}):
        rc, msg = rp(**kw)
        assert rc == TD_ERR_INVALID and "aligned" in msg, (kw, msg)
    for layout in (2, 4, -1):
        rc, msg = rp(layout=layout)
        assert rc == TD_ERR_INVALID and f"layout={layout}" in msg
    rc, msg = rp(G=16)
    assert rc == TD_ERR_INVALID and "G=16" in msg and "32, 64 and 128" in msg
    rc, msg = rp(K=192)
    assert rc == TD_ERR_INVALID and "K=192" in msg and "G=128" in msg
    rc, msg = rp(N=60)
    assert rc == TD_ERR_INVALID and "N=60" in msg and "8" in msg
    rc, msg = rp(N=0)
    assert rc == TD_ERR_INVALID and "N=0" in msg

    def dq(pk=pk, sc=so, zp=zo, G=128, w=w, ldw=256, N=64, K=256):
        return lib.td_dequant_rows_int4(pk, sc, zp, G, w, ldw, N, K, None), lib.td_last_error().decode()

    for kw in ({"pk": None}, {"sc": None}, {"zp": None}, {"w": None}):
        rc, msg = dq(**kw)
        assert rc == TD_ERR_INVALID and "required" in msg, (kw, msg)
    for kw in ({"w": w_odd}, {"pk": pk_odd}, {"sc": sc_odd}):
        rc, msg = dq(**kw)
        assert rc == TD_ERR_INVALID and "aligned" in msg, (kw, msg)
    rc, msg = dq(G=100)
    assert rc == TD_ERR_INVALID and "G=100" in msg
    rc, msg = dq(K=320, ldw=320)
    assert rc == TD_ERR_INVALID and "K=320" in msg and "G=128" in msg
    rc, msg = dq(ldw=128)
    assert rc == TD_ERR_INVALID and "ldw" in msg


def test_engine_entry_checks_its_arguments_before_the_handle():
    lib = _lib()
    keep, fake = _buf(1 << 14)      # G and the pointers are checked before the handle is looked at: a zeroed stand-in is never dereferenced
    keep2, buf = _buf(1 << 12)
    keep3, odd = _buf(1 << 12, offset=2)
    name = b"model.layers.0.self_attn.o_proj.weight"
    rc = lib.td_qwen2_load_param_int4(fake, name, buf, buf, buf, 48, None)
    msg = lib.td_last_error().decode()
    assert rc == TD_ERR_INVALID and "G=48" in msg and "32, 64 and 128" in msg
    for args in ((None, name, buf, buf, buf), (fake, None, buf, buf, buf), (fake, name, None, buf, buf), (fake, name, buf, None, buf), (fake, name, buf, buf, None)):
        assert lib.td_qwen2_load_param_int4(*args, 128, None) == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    assert lib.td_qwen2_load_param_int4(fake, name, odd, buf, buf, 128, None) == TD_ERR_INVALID and "aligned" in lib.td_last_error().decode()
    rc = lib.td_qwen2_set_int4_routing(fake, 2)
    assert rc == TD_ERR_INVALID and "all=2" in lib.td_last_error().decode()
    assert lib.td_qwen2_set_int4_routing(None, 1) == TD_ERR_INVALID and "null handle" in lib.td_last_error().decode()
    # there is no round-to-nearest int4 quantiser: mode 3 is not one td_qwen2_quantize_weights takes
    rc = lib.td_qwen2_quantize_weights(fake, 3, None)
    msg = lib.td_last_error().decode()
    assert rc == TD_ERR_INVALID and "mode 3" in msg and "TD_QWEN2_WEIGHTS_E4M3" in msg and "TD_QWEN2_WEIGHTS_MXFP4" in msg


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,G", [(8, 32, 32), (24, 256, 64), (64, 1536, 128)])
def test_checkpoint_layouts_round_trip(N, K, G):
    q, z, s = C.edge_problem(N, K, G, seed=N + K)
    a = C.pack_awq(q, z, s)
    assert a["qweight"].shape == (K, N // 8) and a["qzeros"].shape == (K // G, N // 8) and a["scales"].shape == (K // G, N)
    assert a["qweight"].dtype == a["qzeros"].dtype == torch.int32 and a["scales"].dtype == torch.float16
    for got, want in zip(C.unpack_awq(a), (q, z, s)):
        assert torch.equal(got, want)
    for v2 in (False, True):
        t = C.pack_gptq(q, z, s, v2=v2)
        assert t["qweight"].shape == (K // 8, N) and t["qzeros"].shape == (K // G, N // 8) and t["scales"].shape == (K // G, N)
        assert torch.equal(t["g_idx"], (torch.arange(K) // G).to(torch.int32))
        for got, want in zip(C.unpack_gptq(t, v2=v2), (q, z, s)):
            assert torch.equal(got, want)
    # the definitions themselves, on single words
    k, c, p = 5, 0, 3                                        # AWQ: nibble p of column c holds q[k, 8 c + o[p]]
    assert (int(a["qweight"][k, c]) >> (4 * p)) & 15 == int(q[8 * c + C.AWQ_ORDER[p], k])
    r, n, p = 2, 1, 6                                        # GPTQ: nibble p of row r holds q[8 r + p, n]
    t = C.pack_gptq(q, z, s)
    assert (int(t["qweight"][r, n]) >> (4 * p)) & 15 == int(q[n, 8 * r + p])
    assert (int(t["qzeros"][0, 0]) >> (4 * 5)) & 15 == (int(z[5, 0]) - 1) & 15          # ... and z[g, 8 c + p] - 1
    assert (int(C.pack_gptq(q, z, s, v2=True)["qzeros"][0, 0]) >> (4 * 5)) & 15 == int(z[5, 0])


def test_w_hat_is_one_rounding_of_an_exact_product():
    q, z, s = C.edge_problem(64, 1536, 128, seed=1)
    pairs = {(int(a), int(b)) for a, b in zip(q.flatten().tolist(), z.repeat_interleave(128, dim=1).flatten().tolist())}
    assert len(pairs) == 256
    wh = C.w_hat(q, z, s, 128)
    exact = (q.double() - z.double().repeat_interleave(128, dim=1)) * s.double().repeat_interleave(128, dim=1)
    assert torch.equal(exact.float().double(), exact)                         # the fp32 product IS the product
    assert torch.equal(wh, exact.bfloat16()) and bool(torch.isfinite(wh.float()).all())
    tiny = s.float().abs()[(s != 0)].min()
    assert float(tiny) == 2.0 ** -24                                          # an fp16 subnormal scale ...
    assert float(C.w_hat(torch.tensor([[1]], dtype=torch.uint8).expand(1, 32), torch.zeros(1, 1, dtype=torch.uint8), torch.tensor([[2.0 ** -24]]).half(), 32)[0, 0]) == 2.0 ** -24


# ---- Python: the loader ------------------------------------------------------------------------------------------------------------------------
NAME = "model.layers.0.self_attn.o_proj"
AWQ_CFG = {"quant_method": "awq", "bits": 4, "group_size": 32, "version": "gemm", "zero_point": True}
GPTQ_CFG = {"quant_method": "gptq", "bits": 4, "group_size": 32, "desc_act": False, "sym": True}


def _stand_in(cfg, quantization=None):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine as E
    return types.SimpleNamespace(int4_config=cfg, weight_quantization=quantization, device="cpu", INT4_LINEARS=E.INT4_LINEARS, INT4_TENSORS=E.INT4_TENSORS,
                                 check_int4_config=E.check_int4_config)


def _triple(layout, N=64, K=64, G=32):
    q, z, s = C.edge_problem(N, K, G, seed=3)
    return {NAME + "." + k: v for k, v in C.pack(layout, q, z, s).items()}


def test_int4_loader_refuses_by_key_or_field():
    """Every refusal of load_state_dict's int4 path, raised on the host before anything touches the device (the stand-in has no handle at all)."""
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine as E
    split = E._split_int4
    OTHER = "model.layers.0.mlp.router_proj"      # a Linear of the table that is none of the seven a checkpoint quantises
    table = {NAME + ".weight": 64 * 64, "model.norm.weight": 64, "lm_head.weight": 320 * 64, OTHER + ".weight": 64 * 64}
    awq, gptq = _triple(C.LAYOUT_AWQ), _triple(C.LAYOUT_GPTQ)
    # what passes: one job per Linear, the int4 tensors taken out of the dict
    rest, jobs = split(_stand_in(AWQ_CFG), {**awq, "model.norm.weight": torch.ones(64)}, table)
    assert list(rest) == ["model.norm.weight"] and [(j[0], j[1], j[2]) for j in jobs] == [(NAME + ".weight", C.LAYOUT_AWQ, 32)]
    rest, jobs = split(_stand_in(GPTQ_CFG), gptq, table)
    assert not rest and [(j[0], j[1]) for j in jobs] == [(NAME + ".weight", C.LAYOUT_GPTQ)]
    assert split(_stand_in({**GPTQ_CFG, "checkpoint_format": "gptq_v2"}), gptq, table)[1][0][1] == C.LAYOUT_GPTQ_V2
    sd = {NAME + ".weight": torch.zeros(64, 64)}
    assert split(_stand_in(None), sd, table) == (sd, [])                      # nothing int4: the dict passes through untouched

    def refused(match, cfg, sd, quantization=None):
        with pytest.raises(ValueError, match=match):
            split(_stand_in(cfg, quantization), sd, table)

    # a triple with a member missing
    for member in ("qweight", "qzeros", "scales"):
        refused(re.escape(NAME + "." + member), AWQ_CFG, {k: v for k, v in awq.items() if not k.endswith(member)})
    # wrong dtypes or shapes
    refused(re.escape(NAME + ".qweight") + ".*int32", AWQ_CFG, {**awq, NAME + ".qweight": awq[NAME + ".qweight"].to(torch.int64)})
    refused(re.escape(NAME + ".qweight") + ".*shape", AWQ_CFG, {**awq, NAME + ".qweight": awq[NAME + ".qweight"][:32]})
    refused(re.escape(NAME + ".qzeros"), GPTQ_CFG, awq)       # an AWQ triple read as GPTQ: [64, 8] could be [K / 8, N] of a 512 x 8 Linear, its qzeros could not
    refused(re.escape(NAME + ".qzeros"), AWQ_CFG, {**awq, NAME + ".qzeros": awq[NAME + ".qzeros"][:1]})
    refused(re.escape(NAME + ".qzeros"), AWQ_CFG, {**awq, NAME + ".qzeros": awq[NAME + ".qzeros"].to(torch.int16)})
    refused(re.escape(NAME + ".scales") + ".*shape", AWQ_CFG, {**awq, NAME + ".scales": awq[NAME + ".scales"][:, :32]})
    # scales that are not float16
    refused(re.escape(NAME + ".scales") + ".*float16", AWQ_CFG, {**awq, NAME + ".scales": awq[NAME + ".scales"].bfloat16()})
    refused(re.escape(NAME + ".scales") + ".*float16", AWQ_CFG, {**awq, NAME + ".scales": awq[NAME + ".scales"].float()})
    # the config, field by field
    refused("'bits'", {**AWQ_CFG, "bits": 8}, awq)
    refused("'bits'", {**GPTQ_CFG, "bits": 3}, gptq)
    for G in (16, 256, -1, None):
        refused("'group_size'", {**AWQ_CFG, "group_size": G}, awq)
    refused("'version'", {**AWQ_CFG, "version": "gemv"}, awq)
    refused("'zero_point'", {**AWQ_CFG, "zero_point": False}, awq)
    refused("'desc_act'", {**GPTQ_CFG, "desc_act": True}, gptq)
    refused("'checkpoint_format'", {**GPTQ_CFG, "checkpoint_format": "marlin"}, gptq)
    refused("'quant_method'", {**AWQ_CFG, "quant_method": "bitsandbytes"}, awq)
    # a g_idx that is not k // G
    bad_idx = gptq[NAME + ".g_idx"].clone()
    bad_idx[[3, 40]] = bad_idx[[40, 3]]
    refused(re.escape(NAME + ".g_idx"), GPTQ_CFG, {**gptq, NAME + ".g_idx": bad_idx})
    refused(re.escape(NAME + ".g_idx"), GPTQ_CFG, {**gptq, NAME + ".g_idx": gptq[NAME + ".g_idx"][:32]})
    # a non-finite scale
    for bad in (float("inf"), float("nan")):
        sc = awq[NAME + ".scales"].clone()
        sc[1, 5] = bad
        refused(re.escape(NAME + ".scales") + ".*non-finite", AWQ_CFG, {**awq, NAME + ".scales": sc})
    # int4 tensors for a Linear that is not one of the decoder's seven
    refused(re.escape(OTHER + ".qweight") + ".*decoder Linears", AWQ_CFG, {k.replace(NAME, OTHER): v for k, v in awq.items()})
    # a quantised lm_head
    head = {k.replace(NAME, "lm_head"): v for k, v in awq.items()}
    refused("lm_head.*quantised lm_head", AWQ_CFG, {**awq, **head})
    # int4 tensors without int4_config, and together with a weight quantisation
    refused(re.escape(NAME + ".qweight") + ".*int4_config", None, awq)
    for other in ("fp8", "mxfp4"):
        refused("weight_quantization='" + other + "'", AWQ_CFG, awq, quantization=other)
    # the same Linear twice
    refused(re.escape(NAME + ".weight") + ".*both", AWQ_CFG, {**awq, NAME + ".weight": torch.zeros(64, 64)})


def test_quantization_config_is_read_from_config_json(tmp_path):
    """load_pretrained takes `quantization_config` from the config.json beside the shards (quant_method awq / gptq) -- and refuses an unserved one by field --
    before it reads a tensor: the stand-in has no handle, and the shard here holds nothing the loader would get to."""
    from safetensors.torch import save_file
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine as E
    save_file({"visual.patch_embed.proj.weight": torch.zeros(4)}, str(tmp_path / "model.safetensors"))

    class Stop(Exception):
        pass

    def run(config):
        with open(tmp_path / "config.json", "w") as fh:
            json.dump(config, fh)
        eng = _stand_in(None)
        eng.config = types.SimpleNamespace(tie_word_embeddings=True)

        def load_state_dict(sd, strict=True):
            raise Stop(sorted(sd))
        eng.load_state_dict = load_state_dict
        eng.param_table = lambda: {}
        eng._requantize = lambda: None
        try:
            E.load_pretrained(eng, str(tmp_path))
        except Stop as stop:
            assert stop.args[0] == []                                   # visual.* is skipped
        return eng.int4_config

    assert run({"model_type": "qwen2_vl", "quantization_config": AWQ_CFG}) == AWQ_CFG
    assert run({"quantization_config": {**GPTQ_CFG, "group_size": 128}})["quant_method"] == "gptq"
    assert run({"model_type": "qwen2_vl"}) is None
    assert run({"quantization_config": {"quant_method": "fp8"}}) is None      # not an int4 checkpoint: none of this loader's business
    with pytest.raises(ValueError, match="'desc_act'"):
        run({"quantization_config": {**GPTQ_CFG, "desc_act": True}})
    with pytest.raises(ValueError, match="'bits'"):
        run({"quantization_config": {**AWQ_CFG, "bits": 8}})


def test_quantization_keyword_is_unchanged_and_points_at_detection():
    from thinkdiff import _hip
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine as E
    for word in ("awq", "gptq", "int4"):
        with pytest.raises(ValueError, match="'" + word + "'.*'fp8'.*quantization_config.*quantization left unset"):
            E.check_quantization(word)
    assert "int4" not in E.WEIGHT_QUANTIZATIONS and _hip.QWEN2_WEIGHTS_INT4 not in E.WEIGHT_QUANTIZATIONS.values()
    with pytest.raises(ValueError, match="'int4'"):
        E.quantize_weights(object(), "int4")
