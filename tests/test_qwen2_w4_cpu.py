"""The MXFP4 weight stream of the Qwen2-VL decode engine without a GPU: the format's CPU restatement (tests/qwen2_w4_common.py) and its properties,
the exported / declared / bound symbols, the ABI version, the C ABI's argument errors (TD_ERR_INVALID with a message, before any HIP call), the models'
`vllm_config["quantization"] = "mxfp4"` and the pre-quantised loader's refusals."""
import ctypes
import os
import re
import types

import pytest
import torch

import qwen2_w4_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
HEADER = os.path.join(ROOT, "include", "thinkdiff_hip.h")
TD_ERR_INVALID = 2

SYMBOLS = ["td_quant_weight_rows_mxfp4", "td_dequant_rows_mxfp4", "td_linear_w4_bf16", "td_linear_split_w4_bf16", "td_linear_glu_w4_bf16"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def test_ties_saturation_and_signed_zero():
    w = torch.zeros(1, 32)
    w[0, :7] = torch.tensor(C.TIES)
    w[0, 7] = 7.0                                  # amax = 7: e = floor(log2 7) - 2 = 0
    w[0, 8:15] = -torch.tensor(C.TIES)
    w[0, 15], w[0, 16], w[0, 17] = -7.0, -0.0, 6.0
    packed, scales, w_hat, e = C.quantize_blocks(w)
    assert int(e[0, 0]) == 0 and int(scales[0, 0]) == 127
    assert w_hat[0, :8].tolist() == list(C.TIES_ROUNDED) + [6.0]
    assert w_hat[0, 8:16].tolist() == [-v for v in C.TIES_ROUNDED] + [-6.0]
    codes = C.unpack(packed)[0]
    assert codes[:8].tolist() == [0, 2, 2, 4, 4, 6, 6, 7] and codes[8:16].tolist() == [8, 10, 10, 12, 12, 14, 14, 15]
    assert int(codes[16]) == 8 and int(codes[17]) == 7 and int(codes[18]) == 0                  # -0 keeps its sign bit
    assert int(packed[0, 0]) == 0 | (2 << 4)                                                    # element 0 in the LOW nibble


def test_exponent_rule_and_clamp():
    w = torch.zeros(6, 32)
    w[0, 3] = 4.0 * 2.0 ** -3       # exactly 4 x 2^e
    w[1, 3] = -6.0 * 2.0 ** 4       # exactly 6 x 2^e
    w[2, 3] = 7.5                   # in (6, 8) x 2^0: clips to 6
    w[3, 3] = 1.5 * 2.0 ** -70      # clamps at -64
    w[4, 3], w[4, 4] = 2.0 ** 70, 3.0 * 2.0 ** 64   # clamps at +64
    _, scales, w_hat, e = C.quantize_blocks(w)
    assert e[:, 0].tolist() == [-3, 4, 0, -64, 64, 0]
    assert scales[:, 0].tolist() == [124, 131, 127, 63, 191, 127]
    assert float(w_hat[0, 3]) == 0.5 and float(w_hat[1, 3]) == -96.0 and float(w_hat[2, 3]) == 6.0
    assert float(w_hat[3, 3]) == 0.0 and float(w_hat[4, 3]) == 6.0 * 2.0 ** 64 and float(w_hat[4, 4]) == 3.0 * 2.0 ** 64
    assert not w_hat[5].any()


@pytest.mark.parametrize("N,K", [(4, 32), (19, 1536), (64, 8960)])
def test_restatement_properties(N, K):
    w = C.edge_blocks(N, K, seed=N + K)
    packed, scales, w_hat, e = C.quantize_blocks(w)
    assert packed.shape == (N, K // 2) and scales.shape == (N, K // 32) and packed.dtype == scales.dtype == torch.uint8
    assert torch.equal(w_hat.bfloat16().float(), w_hat)                                   # W^ is a bf16 value exactly
    assert torch.equal(C.dequantize(packed, scales), w_hat)
    # idempotent: the same bytes and scales -- a block's maximum rounds to 4 x 2^e or 6 x 2^e of its own exponent, never out of it (a block that rounded to
    # zero, under the -64 clamp, is a zero block the second time: scale byte 127)
    p2, s2, w2, _ = C.quantize_blocks(w_hat)
    zeroed = (w_hat.view(N, -1, 32) == 0).all(2)
    assert torch.equal(w2, w_hat) and torch.equal(p2, packed)
    assert torch.equal(s2[~zeroed], scales[~zeroed]) and bool((s2[zeroed] == 127).all())
    # a foreign scale rule (every exponent one higher): other bytes, and quantising ITS values under the OCP rule returns those values
    free = (e > C.E_MIN) & (e < C.E_MAX - 1) & ~zeroed
    pf, sf, wf, _ = C.quantize_blocks(w, bump=1)
    assert bool((sf[free] == scales[free] + 1).all())
    p3, s3, w3, _ = C.quantize_blocks(wf)
    assert torch.equal(w3.view(N, -1, 32)[free], wf.view(N, -1, 32)[free])      # (a block at the +64 clamp has no room for the foreign exponent)
    big = (wf.view(N, -1, 32).abs().amax(2) > 0) & free
    assert not torch.equal(p3.view(N, -1, 16)[big], pf.view(N, -1, 16)[big])
    # the error of the format: below 2 x 2^e (a scaled maximum just under 8 clips to 6), and half a grid step -- at most 2^e -- for scaled values up to 6
    err = (w_hat.double() - w.double()).abs().view(N, -1, 32)
    step = torch.exp2(e[free].double())[:, None]
    inside = w.double().abs().view(N, -1, 32)[free] <= 6 * step
    assert bool((err[free] < 2 * step).all()) and bool((err[free][inside] <= step.expand_as(inside)[inside]).all())


def test_edge_blocks_hold_what_they_promise():
    w = C.edge_blocks(19, 32, seed=1).float()
    _, _, w_hat, e = C.quantize_blocks(w)
    assert e[:3, 0].tolist() == [0, 0, -4] and e[4:12, 0].tolist() == [0, 5, -3, 4, -64, 64, 4, -8]
    assert not w[1].any() and int((w[2] != 0).sum()) == 1 and int(torch.signbit(w[3]).logical_and(w[3] == 0).sum()) == 3
    assert float(w_hat[4].abs().max()) == 6.0 and float(w[4].abs().max()) == 7.5
    assert float(w_hat[6].abs().max()) == 0.5 and float(w_hat[7].abs().max()) == 96.0
    assert not w_hat[8].any() and float(w_hat[9, 0]) == 6.0 * 2.0 ** 64


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
    assert re.search(r"TD_QWEN2_WEIGHTS_MXFP4\s*=\s*2", header) and _hip.QWEN2_WEIGHTS_MXFP4 == 2
    assert lib.td_abi_version() >= 20
    for fn in ("quant_weight_rows_mxfp4", "dequant_rows_mxfp4", "linear_w4", "linear_split_w4", "linear_glu_w4"):
        assert callable(getattr(_hip, fn))
    from thinkdiff import ops
    for op in ("quant_weight_rows_mxfp4", "dequant_rows_mxfp4", "linear_w4"):
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


def test_linear_w4_argument_errors_come_before_any_hip_call():
    lib = _lib()
    keep, x = _buf(1 << 16)
    keep2, wq = _buf(1 << 16)
    keep3, sc = _buf(1 << 12)
    keep4, y = _buf(1 << 16)
    keep5, x_odd = _buf(1 << 16, offset=2)
    keep6, wq_odd = _buf(1 << 16, offset=8)
    keep7, sc_odd = _buf(1 << 12, offset=4)

    def call(x=x, ldx=256, wq=wq, sc=sc, y=y, ldy=64, M=4, N=64, K=256):
        return lib.td_linear_w4_bf16(x, ldx, wq, sc, None, y, ldy, M, N, K, 0, None, None, 0, None), lib.td_last_error().decode()

    rc, msg = call(M=65)
    assert rc == TD_ERR_INVALID and "M=65" in msg and "64" in msg
    for kw in ({"x": None}, {"wq": None}, {"sc": None}, {"y": None}):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "required" in msg, (kw, msg)
    for kw in ({"x": x_odd}, {"wq": wq_odd}, {"sc": sc_odd}):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "aligned" in msg, (kw, msg)
    rc, msg = call(K=100, ldx=104)           # K % 32 != 0: not a whole number of MX blocks
    assert rc == TD_ERR_INVALID and "K=100" in msg
    rc, msg = call(M=17, K=384, ldx=384)     # more than 16 rows need the matrix-core form: K % 256 == 0
    assert rc == TD_ERR_INVALID and "K=384" in msg and "256" in msg
    rc, msg = call(N=62)
    assert rc == TD_ERR_INVALID and "N=62" in msg
    rc, msg = call(ldx=128)
    assert rc == TD_ERR_INVALID and "lda=128" in msg
    assert call(M=0)[0] == TD_ERR_INVALID
    # the split and gated entries share the checks
    rc = lib.td_linear_split_w4_bf16(x, 256, wq, sc, None, y, 64, 0, None, 64, 0, 4, 64, 256, 32, None)
    assert rc == TD_ERR_INVALID and "y1" in lib.td_last_error().decode()
    rc = lib.td_linear_split_w4_bf16(x, 256, wq, sc, None, y, 64, 0, y, 64, 0, 4, 64, 256, 30, None)
    assert rc == TD_ERR_INVALID and "split" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_w4_bf16(x, 256, wq, sc, y, 64, 65, 64, 256, None)
    assert rc == TD_ERR_INVALID and "M=65" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_w4_bf16(x, 256, wq, sc, y, 64, 4, 60, 256, None)
    assert rc == TD_ERR_INVALID and "glu" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_w4_bf16(x, 256, None, sc, y, 64, 4, 64, 256, None)
    assert rc == TD_ERR_INVALID and "required" in lib.td_last_error().decode()


def test_quantiser_argument_errors_come_before_any_hip_call():
    lib = _lib()
    keep, w = _buf(1 << 16)
    keep2, q = _buf(1 << 16)
    keep3, sc = _buf(1 << 12)
    keep4, w_odd = _buf(1 << 16, offset=4)
    keep5, q_odd = _buf(1 << 16, offset=4)
    f = lib.td_quant_weight_rows_mxfp4
    assert f(None, 128, q, sc, None, 4, 128, None) == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    assert f(w, 128, None, sc, None, 4, 128, None) == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    assert f(w, 128, q, None, None, 4, 128, None) == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    assert f(w_odd, 128, q, sc, None, 4, 128, None) == TD_ERR_INVALID and "aligned" in lib.td_last_error().decode()
    assert f(w, 128, q, sc, w_odd, 4, 128, None) == TD_ERR_INVALID and "aligned" in lib.td_last_error().decode()
    assert f(w, 128, q_odd, sc, None, 4, 128, None) == TD_ERR_INVALID and "aligned" in lib.td_last_error().decode()
    assert f(w, 104, q, sc, None, 4, 100, None) == TD_ERR_INVALID and "K=100" in lib.td_last_error().decode()
    assert f(w, 64, q, sc, None, 4, 128, None) == TD_ERR_INVALID and "ldw" in lib.td_last_error().decode()
    assert f(w, 128, q, sc, None, 0, 128, None) == TD_ERR_INVALID and "N=0" in lib.td_last_error().decode()
    d = lib.td_dequant_rows_mxfp4
    assert d(None, sc, w, 128, 4, 128, None) == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    assert d(q, None, w, 128, 4, 128, None) == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    assert d(q, sc, None, 128, 4, 128, None) == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    assert d(q, sc, w_odd, 128, 4, 128, None) == TD_ERR_INVALID and "aligned" in lib.td_last_error().decode()
    assert d(q_odd, sc, w, 128, 4, 128, None) == TD_ERR_INVALID and "aligned" in lib.td_last_error().decode()
    assert d(q, sc, w, 104, 4, 100, None) == TD_ERR_INVALID and "K=100" in lib.td_last_error().decode()
    assert d(q, sc, w, 64, 4, 128, None) == TD_ERR_INVALID and "ldw" in lib.td_last_error().decode()


def test_engine_mode_errors_name_both_served_modes():
    lib = _lib()
    keep, fake = _buf(1 << 14)      # the mode is checked before the handle is looked at: a zeroed stand-in is never dereferenced
    rc = lib.td_qwen2_quantize_weights(fake, 7, None)
    msg = lib.td_last_error().decode()
    assert rc == TD_ERR_INVALID and "mode 7" in msg and "TD_QWEN2_WEIGHTS_E4M3" in msg and "TD_QWEN2_WEIGHTS_MXFP4" in msg
    assert lib.td_qwen2_quantize_weights(None, 2, None) == TD_ERR_INVALID


# ---- Python -------------------------------------------------------------------------------------------------------------------------------------
def test_mxfp4_is_a_served_quantization():
    from thinkdiff import _hip
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine
    assert Qwen2VLTextEngine.check_quantization("mxfp4") == "mxfp4"
    assert Qwen2VLTextEngine.WEIGHT_QUANTIZATIONS["mxfp4"] == _hip.QWEN2_WEIGHTS_MXFP4
    with pytest.raises(ValueError, match=r"'nvfp4'.*'fp8'.*'mxfp4'"):
        Qwen2VLTextEngine.check_quantization("nvfp4")
    with pytest.raises(ValueError, match="mxfp4"):
        Qwen2VLTextEngine.quantize_weights(object(), "int4")


def test_prequantised_loader_refuses_by_key():
    """The three refusals of load_state_dict's packed-tensor path, raised before anything touches the device: a packed tensor without its scales, a wrong
    shape, and packed tensors on an engine whose quantisation is not "mxfp4"."""
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine
    name = "model.layers.0.self_attn.o_proj.weight"
    table = {name: 64 * 64, "model.norm.weight": 64}
    eng = types.SimpleNamespace(weight_quantization="mxfp4", device="cpu", PACKED_LINEARS=Qwen2VLTextEngine.PACKED_LINEARS)
    packed, scales = torch.zeros(64, 32, dtype=torch.uint8), torch.full((64, 2), 127, dtype=torch.uint8)
    prep = Qwen2VLTextEngine._dequantize_packed
    with pytest.raises(ValueError, match=re.escape(name + "_scale")):
        prep(eng, {name: packed}, table)                                                        # no scales
    with pytest.raises(ValueError, match=re.escape(name)):
        prep(eng, {name + "_scale": scales}, table)                                             # scales without a packed tensor
    with pytest.raises(ValueError, match=re.escape(name) + ".*shape"):
        prep(eng, {name: packed[:, :16], name + "_scale": scales}, table)                       # the wrong shape
    with pytest.raises(ValueError, match=re.escape(name + "_scale")):
        prep(eng, {name: packed, name + "_scale": scales[:, :1]}, table)                        # ... of the scales
    with pytest.raises(ValueError, match=re.escape(name + "_scale")):
        prep(eng, {name: packed, name + "_scale": scales.float()}, table)
    for other in (None, "fp8"):
        eng.weight_quantization = other
        with pytest.raises(ValueError, match=re.escape(name) + ".*mxfp4"):
            prep(eng, {name: packed, name + "_scale": scales}, table)
    # nothing packed: the dict passes through untouched
    eng.weight_quantization = None
    sd = {name: torch.zeros(64, 64, dtype=torch.bfloat16)}
    assert prep(eng, sd, table) is sd
