"""The 8-bit weight stream of the Qwen2-VL decode engine without a GPU: the format's CPU restatement (tests/qwen2_w8_common.py) and its invariants,
the exported / declared / bound symbols, the ABI version, the C ABI's argument errors (TD_ERR_INVALID with a message, before any HIP call) and
the models' `vllm_config["quantization"]` key."""
import ctypes
import os
import re

import pytest
import torch

import qwen2_w8_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
HEADER = os.path.join(ROOT, "include", "thinkdiff_hip.h")
PARENT_ABI_VERSION = 11      # td_abi_version() of the commit before the 8-bit weight stream
TD_ERR_INVALID = 2

SYMBOLS = ["td_quant_weight_rows_e4m3", "td_linear_w8_bf16", "td_linear_split_w8_bf16", "td_linear_glu_bf16", "td_linear_glu_w8_bf16",
           "td_qwen2_quantize_weights", "td_qwen2_set_weight_stream", "td_qwen2_weight_info"]


def _f8(x):
    return torch.tensor(x, dtype=torch.float32).to(torch.float8_e4m3fn).float()


def test_torch_cpu_e4m3_conversion_is_what_the_restatement_assumes():
    # round to nearest even on the 3-bit mantissa: 17 (tie between 16 and 18) -> 16, 19 (tie between 18 and 20) -> 20, 21 -> 20 (tie) ...
    assert _f8([17.0, 19.0, 21.0, 23.0, 18.5, 17.5]).tolist() == [16.0, 20.0, 20.0, 24.0, 18.0, 18.0]
    # subnormals: the smallest is 2^-9; 2^-10 is a tie with 0 and goes to 0 (even), 1.5 x 2^-9 is a tie between 2^-9 and 2^-8 and goes to 2^-8 (even)
    assert _f8([2.0 ** -10, 1.5 * 2.0 ** -9, 2.0 ** -9, 0.75 * 2.0 ** -9]).tolist() == [0.0, 2.0 ** -8, 2.0 ** -9, 2.0 ** -9]
    # the largest value is 448 (the step there is 32); up to the tie at 464 a value rounds to 448 (even), NaN only above -- the scale rule keeps
    # every scaled weight at or below 448
    got = _f8([448.0, 460.0, 464.0])
    assert got.tolist() == [448.0, 448.0, 448.0]
    assert torch.isnan(_f8([466.0, 480.0])).all()
    assert _f8([-448.0, -0.0, 0.0]).tolist() == [-448.0, 0.0, 0.0]


@pytest.mark.parametrize("N,K", [(4, 128), (19, 1536), (64, 8960)])
def test_restatement_invariants(N, K):
    w = C.edge_rows(N, K, seed=N + K)
    q, scale, w_hat, e = C.quantize_rows(w)
    qf = q.view(torch.float8_e4m3fn).float()
    assert not torch.isnan(qf).any() and float(qf.abs().max()) <= 448.0
    assert torch.equal(w_hat.bfloat16().float(), w_hat)                    # W^ is a bf16 value exactly
    # e_n is the SMALLEST exponent that fits (unless clamped): amax 2^-e <= 448 < amax 2^-(e-1)
    amax = w.float().abs().amax(dim=1).double()
    nz = amax > 0
    assert bool((amax * torch.exp2(-e.double()) <= 448.0).all())
    free = nz & (e > C.E_MIN) & (e < C.E_MAX)
    assert bool((amax[free] * torch.exp2(-(e[free].double() - 1)) > 448.0).all())
    assert int(e[0]) == 0 and float(scale[0]) == 1.0 and not w_hat[0].any()          # the all-zero row
    assert int((w_hat[1] != 0).sum()) == 1                                            # the single non-zero survives
    assert int(e[2]) == 3 and float(qf[2].abs().max()) == 448.0                       # a maximum of exactly 448 x 2^3 gets e = 3
    assert int(e[3]) == 4
    # quantising W^ returns W^ (the exponent may drop by one where the maximum rounded down to 224 2^e: the bytes double, W^ does not move)
    q2, scale2, w_hat2, e2 = C.quantize_rows(w_hat)
    assert torch.equal(w_hat2, w_hat)
    assert bool(((e2 == e) | (e2 == e - 1) | ~nz).all())
    assert torch.equal(C.dequantize(q, scale), w_hat)
    # the error of the format: at most 2^-4 relative for normal values (3 mantissa bits), 2^-10 x 2^e absolute below
    err = (w_hat.double() - w.double()).abs()
    bound = torch.maximum(w.double().abs() * 2.0 ** -4, (2.0 ** -10 * scale.double())[:, None])
    assert bool((err <= bound).all())


def test_symbols_are_exported_declared_and_bound():
    lib = ctypes.CDLL(LIB)
    header = open(HEADER).read()
    from thinkdiff import _hip
    sig = _hip._declare(lib)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/thinkdiff_hip.h"
        assert name in sig, f"{name} is not bound in thinkdiff/_hip.py"
    assert "TD_QWEN2_WEIGHTS_E4M3" in header
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine
    assert hasattr(lib, "td_qwen2_weight_stream_launches") and "td_qwen2_weight_stream_launches(" in header
    assert lib.td_qwen2_weight_stream_launches.restype is ctypes.c_int64 and lib.td_qwen2_weight_stream_launches(None) == -1
    for m in ("quantize_weights", "set_weight_stream", "weight_info", "weight_stream_launches"):
        assert callable(getattr(Qwen2VLTextEngine, m))


def test_abi_version_moved():
    lib = ctypes.CDLL(LIB)
    assert lib.td_abi_version() > PARENT_ABI_VERSION


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


def test_linear_w8_argument_errors_come_before_any_hip_call():
    lib = _lib()
    keep, x = _buf(1 << 16)
    keep2, wq = _buf(1 << 16)
    keep3, sc = _buf(1 << 12)
    keep4, y = _buf(1 << 16)
    _, x_odd = _buf(1 << 16, offset=2)
    _, wq_odd = _buf(1 << 16, offset=8)

    def call(x=x, ldx=256, wq=wq, sc=sc, y=y, ldy=64, M=4, N=64, K=256):
        return lib.td_linear_w8_bf16(x, ldx, wq, sc, None, y, ldy, M, N, K, 0, None, None, 0, None), lib.td_last_error().decode()

    rc, msg = call(M=65)
    assert rc == TD_ERR_INVALID and "M=65" in msg and "64" in msg
    for kw in ({"x": None}, {"wq": None}, {"sc": None}, {"y": None}):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "required" in msg, (kw, msg)
    for kw in ({"x": x_odd}, {"wq": wq_odd}):
        rc, msg = call(**kw)
        assert rc == TD_ERR_INVALID and "aligned" in msg, (kw, msg)
    rc, msg = call(K=200, ldx=200)           # K % 16 != 0: not a whole number of 16-byte chunks of weight bytes
    assert rc == TD_ERR_INVALID and "K=200" in msg
    rc, msg = call(M=17, K=192, ldx=192)     # more than 16 rows need the matrix-core form: K % 128 == 0
    assert rc == TD_ERR_INVALID and "K=192" in msg and "128" in msg
    rc, msg = call(N=62)
    assert rc == TD_ERR_INVALID and "N=62" in msg
    rc, msg = call(M=0)
    assert rc == TD_ERR_INVALID
    # the split and gated entries share the checks
    rc = lib.td_linear_split_w8_bf16(x, 256, wq, sc, None, y, 64, 0, None, 64, 0, 4, 64, 256, 32, None)
    assert rc == TD_ERR_INVALID and "y1" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_w8_bf16(x, 256, wq, sc, y, 64, 65, 64, 256, None)
    assert rc == TD_ERR_INVALID and "M=65" in lib.td_last_error().decode()
    rc = lib.td_linear_glu_bf16(x, 256, None, y, 64, 4, 64, 256, None)
    assert rc == TD_ERR_INVALID and "required" in lib.td_last_error().decode()


def test_quantiser_argument_errors_come_before_any_hip_call():
    lib = _lib()
    keep, w = _buf(1 << 16)
    keep2, q = _buf(1 << 16)
    keep3, sc = _buf(1 << 12)
    _, w_odd = _buf(1 << 16, offset=4)
    f = lib.td_quant_weight_rows_e4m3
    assert f(None, 128, q, sc, None, 4, 128, None) == TD_ERR_INVALID and "required" in lib.td_last_error().decode()
    assert f(w, 128, None, sc, None, 4, 128, None) == TD_ERR_INVALID
    assert f(w, 128, q, None, None, 4, 128, None) == TD_ERR_INVALID
    assert f(w_odd, 128, q, sc, None, 4, 128, None) == TD_ERR_INVALID and "aligned" in lib.td_last_error().decode()
    assert f(w, 128, q, sc, w_odd, 4, 128, None) == TD_ERR_INVALID and "aligned" in lib.td_last_error().decode()
    assert f(w, 128, q, sc, None, 4, 100, None) == TD_ERR_INVALID and "K=100" in lib.td_last_error().decode()
    assert f(w, 64, q, sc, None, 4, 128, None) == TD_ERR_INVALID and "ldw" in lib.td_last_error().decode()


def test_engine_entries_refuse_bad_handles_and_modes():
    lib = _lib()
    # the mode is checked before the handle is looked at: a zeroed stand-in is never dereferenced
    keep, fake = _buf(1 << 14)
    rc = lib.td_qwen2_quantize_weights(fake, 7, None)
    msg = lib.td_last_error().decode()
    assert rc == TD_ERR_INVALID and "mode 7" in msg and "TD_QWEN2_WEIGHTS_E4M3" in msg
    assert lib.td_qwen2_quantize_weights(None, 1, None) == TD_ERR_INVALID
    assert lib.td_qwen2_set_weight_stream(None, 1) == TD_ERR_INVALID
    assert lib.td_qwen2_weight_info(None, None, None, None, None) == TD_ERR_INVALID


@pytest.mark.parametrize("cls_path", ["thinkdiff.models.mllama_vllm_t5_embed_decoder_2:MllamaVllmT5EmbedDecoderForConditionalGeneration_5",
                                      "thinkdiff.models.mllama_vllm_generate_1:MllamaVllmGenerate_1"])
def test_unknown_quantization_is_a_value_error(cls_path):
    import importlib
    mod, name = cls_path.split(":")
    cls = getattr(importlib.import_module(mod), name)
    with pytest.raises(ValueError, match=r"'awq'.*'fp8'"):
        cls(vllm_config={"quantization": "awq", "max_model_len": 64})      # refused before the engine allocates anything


def test_engine_quantize_weights_names_the_one_served():
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine
    with pytest.raises(ValueError, match="fp8"):
        Qwen2VLTextEngine.quantize_weights(object(), "int8")
    assert Qwen2VLTextEngine.check_quantization(None) is None and Qwen2VLTextEngine.check_quantization("fp8") == "fp8"
