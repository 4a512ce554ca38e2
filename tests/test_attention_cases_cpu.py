"""The inputs of tests/test_attention_packed_gpu.py are decisive, and the entries that test adds refuse bad arguments -- both without a GPU.

Decisiveness: for every case of tests/attention_cases_common.py the float64 reference is recomputed under each plausible masking / indexing
mistake (the mutants) and must lie >= 10x the GPU test's bar (2^-7 max|ref| of the segment or batch entry) from the true reference, the way
test_attention_bias_dense checks its bias.  A kernel that makes one of these mistakes therefore misses the bar by a factor of about ten at
least, whatever its rounding.  Measured margins (float64, x the bar; smallest over the places where the mutant applies .. largest):
  packed (Hq, Hkv) = (4, 2): one key more 84 .. 224, one key fewer 91 .. 200, sees the row before its start 102 .. 192, full attention
    123 .. 180, kv head = head % Hkv 126 .. 198
  packed (7, 1): one key more 123 .. 230, one key fewer 113 .. 214, sees the row before its start 110 .. 209, full attention 129 .. 220
    (head % Hkv is the true map when Hkv = 1)
  cached prefill, smallest of the two batch entries: (2, 300) offset+1 159, offset-1 121, first key dropped 159; (17, 64) 116, 132, 115;
    (33, 65) 158, 182, 156; (256, 1029) 150, 154, 134; (257, 320) 152, 201, 141
"""
import ctypes
import os

import pytest

import attention_cases_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "thinkdiff-mlre_amd", "lib", "libthinkdiff_hip.so")


@pytest.mark.parametrize("Hq,Hkv", C.PACKED_HEADS)
def test_packed_plants_are_disjoint_and_cover_the_edges(Hq, Hkv):
    """Per segment: the two row sets are disjoint, no key is owned by two plants, the last row is a successor row and the one before it a
    diagonal row; in THIS launch every offset of 31, 32, 63, 64, 255, 256 carries both kinds, each in a segment in which the offset is an inner
    row (not one of the segment's last two, which carry their kind anyway)."""
    inner = {kind: set() for kind in ("succ", "diag")}
    for n, (succ, diag) in zip(C.PACKED_LENS, C.packed_plants(Hq, Hkv)):
        assert not set(succ) & set(diag)
        keys = [r + 1 for r in succ] + list(diag)
        assert len(keys) == len(set(keys))
        assert n - 1 in succ and all(0 <= r < n for r in succ) and all(1 <= r < n for r in diag)
        assert n < 3 or n - 2 in diag
        inner["succ"] |= {r for r in succ if r < n - 2}
        inner["diag"] |= {r for r in diag if r < n - 2}
    for r in C.PACKED_EDGES:
        assert r in inner["succ"] and r in inner["diag"], r


@pytest.mark.parametrize("Hq,Hkv", C.PACKED_HEADS)
def test_packed_causal_mutants_move_the_reference(Hq, Hkv):
    case = C.packed_case(Hq, Hkv)
    margins = C.packed_margins(case)
    want = {"one key more", "one key fewer", "sees the row before its start", "full attention"} | ({"kv head = head % Hkv"} if Hkv > 1 else set())
    assert set(margins) == want
    n_seg = len(C.PACKED_LENS)
    assert len(margins["one key more"]) == sum(len(s) for s, _ in case["plants"]) >= n_seg
    assert len(margins["one key fewer"]) == sum(len(d) for _, d in case["plants"]) >= n_seg - 3
    assert len(margins["sees the row before its start"]) == n_seg - 1 and len(margins["full attention"]) == sum(n > 1 for n in C.PACKED_LENS)
    for name, places in margins.items():
        lo = min(places, key=lambda t: t[1])
        print(f"packed Hq={Hq} Hkv={Hkv}: mutant '{name}': {min(m for _, m in places):.1f} .. {max(m for _, m in places):.1f} x the bar over "
              f"{len(places)} places (smallest at {lo[0]})")
        for where, m in places:
            assert m >= C.MIN_MARGIN, f"inputs too weak: mutant '{name}' at {where} only {m:.2f} x the bar away"


@pytest.mark.parametrize("Sq,Skv", C.PREFILL_SHAPES)
def test_cached_prefill_mutants_move_the_reference(Sq, Skv):
    case = C.prefill_case(Sq, Skv)
    assert case["succ"] and case["diag"] and case["first"] not in case["succ"]
    margins = C.prefill_margins(case)
    assert set(margins) == {"causal_offset + 1", "causal_offset - 1", "first key dropped"}
    for name, per_batch in margins.items():
        print(f"cached prefill ({Sq}, {Skv}): mutant '{name}': " + ", ".join(f"{m:.1f}" for m in per_batch) + " x the bar per batch entry")
        for b, m in enumerate(per_batch):
            assert m >= C.MIN_MARGIN, f"inputs too weak: mutant '{name}' only {m:.2f} x the bar away in batch entry {b}"


def _lib():
    assert os.path.exists(LIB), "build first: make -C thinkdiff-mlre_amd (or __graft_entry__.build())"
    lib = ctypes.CDLL(LIB)
    lib.td_last_error.restype = ctypes.c_char_p
    return lib


def test_abi_version_and_binding_are_in_step():
    from thinkdiff import _hip
    lib = _hip.lib()
    assert lib.td_abi_version() >= 17
    assert hasattr(lib, "td_attention_segments_bf16") and lib.td_attention_segments_bf16.argtypes is not None
    assert "td_attention_segments_bf16" in open(os.path.join(ROOT, "include", "thinkdiff_hip.h")).read()


def test_attention_segments_refusals_come_before_any_hip_call():
    """Every refusal of td_attention_segments_bf16 is TD_ERR_INVALID with its own message on a machine without a GPU, so it precedes the first HIP
    call: an empty segment list, Hq % Hkv != 0, misaligned strides or pointers, strides shorter than the heads, causal outside {0, 1}."""
    lib = _lib()
    i64, f32, vp = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    good = dict(q=vp(256), ldq=512, k=vp(512), v=vp(768), ldkv=256, o=vp(1024), ldo=512, seg=vp(2048), n_seg=3, max_len=40, Hq=4, Hkv=2, causal=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.td_attention_segments_bf16(a["q"], i64(a["ldq"]), a["k"], a["v"], i64(a["ldkv"]), a["o"], i64(a["ldo"]), a["seg"], a["n_seg"], a["max_len"],
                                              a["Hq"], a["Hkv"], f32(0.088), a["causal"], None)

    cases = [(dict(seg=None), b"empty segment list"), (dict(n_seg=0), b"empty segment list"), (dict(max_len=0), b"empty segment list"),
             (dict(q=None), b"null operand"), (dict(o=None), b"null operand"),
             (dict(causal=2), b"causal=2"), (dict(causal=-1), b"causal=-1"),
             (dict(Hq=5), b"Hq=5 not a positive multiple of Hkv=2"), (dict(Hkv=0), b"multiple of Hkv=0"),
             (dict(ldq=504), b"shorter than its heads"), (dict(ldkv=128), b"shorter than its heads"), (dict(ldo=2 ** 31), b"32-bit range"),
             (dict(ldq=516), b"ldq=516 and ldkv=256 must be multiples of 8"), (dict(ldkv=260), b"ldkv=260 must be multiples of 8"),
             (dict(ldo=514), b"ldo=514 of 4"),
             (dict(q=vp(264)), b"q, k, v and o must be 16-byte aligned"), (dict(k=vp(520)), b"q, k, v and o must be 16-byte aligned"),
             (dict(v=vp(776)), b"q, k, v and o must be 16-byte aligned"), (dict(o=vp(1032)), b"q, k, v and o must be 16-byte aligned"),
             (dict(seg=vp(2050)), b"seg_starts must be 4-byte aligned")]
    for kw, msg in cases:
        rc = call(**kw)
        assert rc == 2 and msg in lib.td_last_error(), (kw, rc, lib.td_last_error())


def test_softmax_rows_refuses_a_scale_that_is_not_finite_and_positive():
    """td_softmax_rows_launch takes the row maximum over the UNSCALED scores, which is the maximum of scale * s only for scale > 0: zero,
    negative, infinite and NaN scales are TD_ERR_INVALID through both entries, before any HIP call, and the message says why."""
    lib = _lib()
    f32, vp = ctypes.c_float, ctypes.c_void_p
    s, p = vp(4096), vp(8192)
    for scale in (0.0, -0.0, -1.0, -512 ** -0.5, float("inf"), float("-inf"), float("nan")):
        for rc in (lib.td_softmax_rows_f32_bf16(s, p, 3, 64, f32(scale), None), lib.td_softmax_rows_strided_f32_bf16(s, p, 3, 60, 64, f32(scale), None)):
            msg = lib.td_last_error()
            assert rc == 2 and b"finite and greater than 0" in msg and b"maximum is taken over the unscaled scores" in msg, (scale, rc, msg)
