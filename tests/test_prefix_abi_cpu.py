"""The two C entries of automatic prefix caching refuse bad arguments with TD_ERR_INVALID and a message naming the value, before any HIP call: with no
GPU present.  (The refusals of td_qwen2_prefill_packed_prefix_slots that need a handle -- counts, slots, lengths -- are in tests/test_prefix_prefill_gpu.py:
a handle cannot be created without a device.)"""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")
vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(LIB)
    L.td_last_error.restype = ctypes.c_char_p
    L.td_attention_prefix_segments_bf16.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp]
    L.td_qwen2_prefill_packed_prefix_slots.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return L


def test_abi_version(lib):
    assert lib.td_abi_version() >= 23


def test_attention_prefix_segments_refusals(lib):
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 63) & ~63      # a 64-byte aligned host address: never dereferenced, every refusal comes first

    def call(q=a, k=a, v=a, o=a, ldq=512, ldkv=256, ldo=512, starts=a, row0=a, lens=a, n=2, mq=8, mkv=16, Hq=4, Hkv=2):
        rc = lib.td_attention_prefix_segments_bf16(q, k, v, o, ldq, ldkv, ldo, starts, row0, lens, n, mq, mkv, Hq, Hkv, 0.088, None)
        return rc, lib.td_last_error().decode()

    for kw, word in [(dict(starts=None), "empty segment list"), (dict(n=0), "empty segment list (n_seg=0"), (dict(mq=0), "max_q_len=0"),
                     (dict(row0=None), "kv_row0 null, kv_lens set"), (dict(lens=None), "kv_row0 set, kv_lens null"),
                     (dict(mkv=7), "max_kv_len=7 is below max_q_len=8"),
                     (dict(q=None), "null operand"), (dict(k=None), "null operand"), (dict(v=None), "null operand"), (dict(o=None), "null operand"),
                     (dict(Hq=5), "Hq=5 not a positive multiple of Hkv=2"), (dict(Hkv=0), "Hkv=0"),
                     (dict(ldq=504), "ldq=504"), (dict(ldkv=128), "ldkv=128"), (dict(ldo=100), "ldo=100"), (dict(ldq=1 << 31), "outside the 32-bit range"),
                     (dict(ldq=516), "ldq=516 and ldkv=256 must be multiples of 8"), (dict(ldkv=260), "ldkv=260 must be multiples of 8"),
                     (dict(ldo=514), "ldo=514 of 4"),
                     (dict(q=a + 8), "16-byte aligned"), (dict(k=a + 2), "16-byte aligned"), (dict(v=a + 4), "16-byte aligned"), (dict(o=a + 8), "16-byte aligned"),
                     (dict(starts=a + 2), "4-byte aligned"), (dict(row0=a + 1), "4-byte aligned"), (dict(lens=a + 3), "4-byte aligned")]:
        rc, msg = call(**kw)
        assert rc == 2 and word in msg and "td_attention_prefix_segments" in msg, (kw, rc, msg)


def test_prefill_packed_prefix_refuses_null_arguments(lib):
    buf = (ctypes.c_int * 16)()
    a = ctypes.addressof(buf)
    # (f, B, slots, token_ids, inputs_embeds, position_ids, lens, prefix_lens, hidden_out, logits_last, stream); the stand-in handle is never dereferenced:
    # the null check is the entry's first statement
    for args in [(None, 1, a, a, None, a, a, a, None, None, None),      # handle
                 (a, 1, None, a, None, a, a, a, None, None, None),      # slots
                 (a, 1, a, None, None, a, a, a, None, None, None),      # neither token_ids nor inputs_embeds
                 (a, 1, a, a, None, None, a, a, None, None, None),      # position_ids
                 (a, 1, a, a, None, a, None, a, None, None, None),      # lens
                 (a, 1, a, a, None, a, a, None, None, None, None)]:     # prefix_lens
        assert lib.td_qwen2_prefill_packed_prefix_slots(*args) == 2 and b"td_qwen2_prefill_packed_prefix: null argument" in lib.td_last_error()


def test_op_schema_and_python_binding():
    import thinkdiff.ops as ops
    ops.register()
    assert str(torch.ops.thinkdiff_hip.attention_prefix_segments.default._schema) == "thinkdiff_hip::attention_prefix_segments" + ops.SCHEMAS["attention_prefix_segments"]
    with pytest.raises((NotImplementedError, RuntimeError)):      # no host kernel to fall back to
        z, i = torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32)
        torch.ops.thinkdiff_hip.attention_prefix_segments(z, z, z, i, i[:1], i[:1], 4, 4, 1, 1, 0.1)
    from thinkdiff import _hip
    assert callable(_hip.attention_prefix_segments)
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine
    for name in ("_prefill_packed_prefix_slots", "prefill_packed", "set_prefix_caching", "reset_prefix_cache", "prefix_cache_stats"):
        assert callable(getattr(Qwen2VLTextEngine, name))
    with pytest.raises(ValueError, match="enable_prefix_caching='yes'"):
        Qwen2VLTextEngine.check_prefix_caching("yes")
    with pytest.raises(ValueError, match="enable_prefix_caching=1 "):
        Qwen2VLTextEngine.check_prefix_caching(1)


@pytest.mark.parametrize("cls_path", ["thinkdiff.models.mllama_vllm_generate_1:MllamaVllmGenerate_1",
                                      "thinkdiff.models.mllama_vllm_t5_embed_decoder_2:MllamaVllmT5EmbedDecoderForConditionalGeneration_5"])
def test_vllm_config_value_is_checked_before_anything_is_allocated(cls_path):
    import importlib
    mod, name = cls_path.split(":")
    cls = getattr(importlib.import_module(mod), name)
    for bad in ("true", 1, None, 0.5):
        with pytest.raises(ValueError, match="enable_prefix_caching"):
            cls(vllm_config={"enable_prefix_caching": bad})
