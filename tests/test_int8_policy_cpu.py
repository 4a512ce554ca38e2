"""The "int8 policy building blocks" entries (include/thinkdiff_hip.h, td_abi_version() >= 7) refuse bad arguments with TD_ERR_INVALID and a
message that names the defect, on a GPU-less host: every check below fails before the launcher's first HIP call (pointers are never dereferenced).
Each case starts from one well-formed argument list per entry and breaks exactly one thing, so a refusal can only come from the check it names."""
import ctypes

import pytest

INVALID = 2
GOOD, OFF4, OFF8 = 4096, 4096 + 4, 4096 + 8          # fake device addresses: 16-byte aligned / only 4-byte / only 8-byte aligned


@pytest.fixture(scope="module")
def L():
    from thinkdiff import _hip
    return _hip.lib()


def _refused(L, rc, *needles):
    msg = L.td_last_error().decode()
    assert rc == INVALID, (rc, msg)
    assert msg and all(n in msg for n in needles), (msg, needles)


def test_abi_version_names_the_int8_policy_blocks(L):
    assert L.td_abi_version() >= 7


# ---- quantising norm ---------------------------------------------------------------------------------------------------------------------
def _norm_args(**kw):
    a = dict(x=GOOD, ldx=1024, q=GOOD, ldq=1024 + 64, q_scale=GOOD, rows=5, D=1024, rms=0, eps=1e-6, w=None, split=2, shiftA=GOOD, scaleA=GOOD, shiftB=GOOD,
             scaleB=GOOD, int8=1, smoothA=GOOD, smoothB=GOOD, extA=GOOD, extB=GOOD, ext_n=64, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,needles", [
    (dict(x=None), ["required"]), (dict(q=None), ["required"]), (dict(q_scale=None), ["required"]),
    (dict(x=OFF8), ["16-byte"]), (dict(smoothB=OFF8), ["16-byte"]), (dict(scaleA=OFF4), ["16-byte"]),
    (dict(q=OFF4), ["misaligned rows", "8-byte"]), (dict(ldq=1024 + 68), ["multiples of 8"]), (dict(ldx=1020), ["multiples of 8"]), (dict(ldx=512), ["ldx >= D"]),
    (dict(ldq=1024 + 56), ["ldq=1080", "D + ext_n = 1088"]), (dict(ldq=1024, ext_n=2), ["ldq=1024", "1026"]),
    (dict(ext_n=63), ["ext_n=63", "even"]),
    (dict(int8=0), ["int8 form only"]),
    (dict(extB=None), ["both tables"]), (dict(ext_n=0), ["both tables"]), (dict(extA=None, extB=None), ["both tables"]),
    (dict(D=1000), ["D=1000"]), (dict(D=4608, ldx=4608, ldq=8192), ["D=4608"]), (dict(rows=0), ["rows=0"]),
    (dict(shiftA=None), ["shift and scale"]), (dict(shiftA=None, scaleA=None), ["shift and scale"]),
])
def test_norm_rows_quant8_refusals(L, kw, needles):
    _refused(L, L.td_norm_rows_quant8(*_norm_args(**kw)), "td_norm_rows_quant8", *needles)


# ---- row quantiser and the smoothing helpers --------------------------------------------------------------------------------------------
def _quant_args(**kw):
    a = dict(x=GOOD, ldx=520, q=GOOD, ldq=528, scale=GOOD, rows=5, K=520, int8=1, col_mul=GOOD, amax_out=GOOD, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,needles", [
    (dict(x=None), ["required"]), (dict(q=None), ["required"]), (dict(scale=None), ["required"]),
    (dict(x=OFF8), ["misaligned rows"]), (dict(q=OFF4), ["misaligned rows"]), (dict(col_mul=OFF8), ["misaligned rows", "col_mul"]),
    (dict(K=524), ["K=524"]), (dict(rows=0), ["rows=0"]), (dict(ldx=516), ["ldx=516"]), (dict(ldq=512), ["ldq=512"]), (dict(ldq=524), ["ldq=524"]),
])
def test_quant_rows8_refusals(L, kw, needles):
    _refused(L, L.td_quant_rows8(*_quant_args(**kw)), "td_quant_rows8", *needles)


def test_smoothing_helpers_refusals(L):
    _refused(L, L.td_col_amax_bf16(None, 2048, 64, 2048, GOOD, None), "td_col_amax_bf16", "required")
    _refused(L, L.td_col_amax_bf16(GOOD, 2048, 64, 2048, None, None), "td_col_amax_bf16", "required")
    _refused(L, L.td_col_amax_bf16(OFF8, 2048, 64, 2048, GOOD, None), "td_col_amax_bf16", "misaligned rows")
    _refused(L, L.td_col_amax_bf16(GOOD, 2044, 64, 2048, GOOD, None), "td_col_amax_bf16", "ldx=2044")
    _refused(L, L.td_col_amax_bf16(GOOD, 2048, 64, 2052, GOOD, None), "td_col_amax_bf16", "K=2052")
    _refused(L, L.td_col_amax_bf16(GOOD, 2048, 0, 2048, GOOD, None), "td_col_amax_bf16", "rows=0")
    for i in range(5):
        args = [GOOD, GOOD, 100, GOOD, GOOD, GOOD, None]
        args[i if i < 2 else i + 1] = None
        _refused(L, L.td_smooth_factors(*args), "td_smooth_factors", "required")
    _refused(L, L.td_smooth_factors(GOOD, GOOD, 0, GOOD, GOOD, GOOD, None), "td_smooth_factors", "n=0")
    for i in range(3):
        args = [GOOD, GOOD, GOOD, 255, 1.25, None]
        args[i] = None
        _refused(L, L.td_q8_scales_from_amax(*args), "td_q8_scales_from_amax", "required")
    _refused(L, L.td_q8_scales_from_amax(GOOD, GOOD, GOOD, 0, 1.25, None), "td_q8_scales_from_amax", "n=0")
    for margin in (0.99, 0.0, -1.25, float("nan")):
        _refused(L, L.td_q8_scales_from_amax(GOOD, GOOD, GOOD, 255, margin, None), "td_q8_scales_from_amax", "margin")
    _refused(L, L.td_ext_cols_int8(None, 3200, 5, 3072, GOOD, 128, None), "td_ext_cols_int8", "required")
    _refused(L, L.td_ext_cols_int8(GOOD, 3200, 5, 3072, None, 128, None), "td_ext_cols_int8", "required")
    _refused(L, L.td_ext_cols_int8(GOOD, 3199, 5, 3072, GOOD, 128, None), "td_ext_cols_int8", "ld=3199")
    _refused(L, L.td_ext_cols_int8(GOOD, 3200, 5, 3072, GOOD, 0, None), "td_ext_cols_int8", "ext_n=0")
    _refused(L, L.td_ext_cols_int8(GOOD, 3200, 0, 3072, GOOD, 128, None), "td_ext_cols_int8", "rows=0")


# ---- int8 GEMM with int8 output ------------------------------------------------------------------------------------------------------------
def _problem(**kw):
    from thinkdiff._hip import TdLinearQ8Problem
    f = dict(xq=GOOD, x_scale=GOOD, wq=GOOD, w_scale=GOOD, bias=GOOD, q8=GOOD, q8_inv=GOOD, q8_amax=GOOD, q8_smooth=GOOD, M=65)
    f.update(kw)
    return TdLinearQ8Problem(**f)


Q8_PROBLEM_CASES = [
    (dict(xq=None), ["operands"]), (dict(x_scale=None), ["operands"]), (dict(wq=None), ["operands"]), (dict(w_scale=None), ["operands"]),
    (dict(q8=None), ["q8 is required"]), (dict(q8_inv=None), ["q8_inv"]), (dict(q8_amax=None), ["q8_amax"]),
    (dict(xq=OFF8), ["misaligned rows"]), (dict(q8=OFF8), ["misaligned rows"]), (dict(q8_smooth=OFF8), ["misaligned rows"]), (dict(bias=OFF4), ["misaligned rows"]),
    (dict(M=0), ["M=0"]),
]


@pytest.mark.parametrize("kw,needles", Q8_PROBLEM_CASES)
def test_linear_int8_q8_refuses_a_bad_problem(L, kw, needles):
    good, bad = _problem(), _problem(**kw)
    ref = ctypes.byref
    _refused(L, L.td_linear_int8_q8(ref(bad), 256, 272, 272, 256, 0, 0, None), "td_linear_int8_q8", *needles)
    _refused(L, L.td_linear_split_int8_q8(ref(bad), 256, 512, GOOD, 256, 0, 1, 768, 256, 256, 0, None), "td_linear_split_int8_q8", *needles)
    _refused(L, L.td_linear_grouped2_int8_q8(ref(bad), ref(good), 256, 272, 272, 256, 0, 0, None), "td_linear_grouped2_int8_q8 (problem 0)", *needles)
    _refused(L, L.td_linear_grouped2_int8_q8(ref(good), ref(bad), 256, 272, 272, 256, 0, 0, None), "td_linear_grouped2_int8_q8 (problem 1)", *needles)


def test_linear_int8_q8_refuses_bad_extents(L):
    p = ctypes.byref(_problem())
    one = lambda **kw: L.td_linear_int8_q8(*list({**dict(a=p, ldx=256, ldq8=272, N=272, K=256, act=0, cfg=0, stream=None), **kw}.values()))
    _refused(L, one(a=None), "td_linear_int8_q8", "null problem")
    _refused(L, one(N=264, ldq8=272), "td_linear_int8_q8", "N=264", "multiples of 16")          # N % 8 == 0 is enough for a bf16 output, not for this one
    _refused(L, one(K=192), "td_linear_int8_q8", "K=192")
    _refused(L, one(ldx=248), "td_linear_int8_q8", "ldx=248")
    _refused(L, one(ldq8=256), "td_linear_int8_q8", "ldq8=256")                                   # narrower than the N int8 columns
    _refused(L, one(ldq8=280), "td_linear_int8_q8", "ldq8=280")                                   # rows would not be 16-byte aligned
    _refused(L, one(act=5), "td_linear_int8_q8", "activation")
    for cfg in (3, 1, 4, 7, -2):
        _refused(L, one(cfg=cfg), "td_linear_int8_q8", f"tile_cfg={cfg}")
    split = lambda **kw: L.td_linear_split_int8_q8(*list({**dict(a=p, ldx=256, ldq8=512, y0=GOOD, ldy0=256, act0=0, act1=1, N=768, K=256, n_split=256, cfg=0,
                                                                 stream=None), **kw}.values()))
    _refused(L, split(a=None), "td_linear_split_int8_q8", "null problem")
    for n_split in (0, 768, 128, 264):
        _refused(L, split(n_split=n_split), "td_linear_split_int8_q8", f"n_split={n_split}")
    _refused(L, split(N=776), "td_linear_split_int8_q8", "multiples of 16")                       # 520 int8 columns
    _refused(L, split(ldq8=496), "td_linear_split_int8_q8", "ldq8=496")                           # narrower than the 512 int8 columns
    _refused(L, split(y0=None), "td_linear_split_int8_q8", "y0")
    _refused(L, split(y0=OFF8), "td_linear_split_int8_q8", "y0")
    _refused(L, split(ldy0=248), "td_linear_split_int8_q8", "ldy0=248")
    _refused(L, split(act0=9), "td_linear_split_int8_q8", "activation")
    _refused(L, split(cfg=3), "td_linear_split_int8_q8", "tile_cfg=3")
    _refused(L, L.td_linear_grouped2_int8_q8(p, None, 256, 272, 272, 256, 0, 0, None), "td_linear_grouped2_int8_q8", "two problems")
    _refused(L, L.td_linear_grouped2_int8_q8(p, p, 256, 272, 272, 256, 0, 3, None), "td_linear_grouped2_int8_q8", "tile_cfg=3")


# ---- joint attention with int8 output ----------------------------------------------------------------------------------------------------------
def _attn_args(fp8, **kw):
    a = dict(q=GOOD, ldq=3 * 256, k=GOOD, v=GOOD, ldkv=3 * 256, q8=GOOD, ldq8=256 + 512, q8_inv=GOOD, q8_amax=GOOD, Sq=300, Skv=300, H=2, scale=0.088)
    a.update(dict(workspace=GOOD) if fp8 else dict(causal=0, bias=None, q_prescaled=0, score_bound=0.0))
    a["stream"] = None
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("kw,needles", [
    (dict(q=None), ["q, k and v"]), (dict(k=None), ["q, k and v"]), (dict(v=None), ["q, k and v"]),
    (dict(q8=None), ["q8 is required"]), (dict(q8_inv=None), ["q8_inv"]), (dict(q8_amax=None), ["q8_amax"]),
    (dict(q=OFF8), ["misaligned rows"]), (dict(v=OFF8), ["misaligned rows"]), (dict(q8=OFF4), ["misaligned rows"]),
    (dict(ldq=764), ["ldq=764"]), (dict(ldkv=128), ["ldkv=128"]), (dict(ldq8=252), ["ldq8=252"]), (dict(ldq8=248), ["ldq8=248"]),
    (dict(Sq=0), ["Sq=0"]), (dict(Skv=0), ["Skv=0"]), (dict(H=0), ["H=0"]),
])
def test_attention_q8_refusals(L, fp8, kw, needles):
    fn, name = (L.td_attention_fp8_q8, "td_attention_fp8_q8") if fp8 else (L.td_attention_q8, "td_attention_q8")
    _refused(L, fn(*_attn_args(fp8, **kw)), name, *needles)


def test_attention_q8_refuses_masks_biases_and_loose_bounds(L):
    _refused(L, L.td_attention_q8(*_attn_args(False, causal=1)), "td_attention_q8", "joint attention only")
    _refused(L, L.td_attention_q8(*_attn_args(False, bias=GOOD)), "td_attention_q8", "joint attention only")
    _refused(L, L.td_attention_q8(*_attn_args(False, score_bound=16.0)), "td_attention_q8", "score bound")                  # a bound without pre-scaled q
    _refused(L, L.td_attention_q8(*_attn_args(False, q_prescaled=1, score_bound=49.0)), "td_attention_q8", "score bound")
    _refused(L, L.td_attention_fp8_q8(*_attn_args(True, workspace=None)), "td_attention_fp8_q8", "workspace")
    _refused(L, L.td_attention_fp8_q8(*_attn_args(True, workspace=OFF8)), "td_attention_fp8_q8", "workspace")
