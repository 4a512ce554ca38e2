"""The grouped int4 (AWQ / GPTQ) weight stream of the Qwen2-VL decode engine on the GPU: repack + dequantise bit for bit against the CPU restatement
(tests/qwen2_int4_common.py) for both checkpoint layouts, the int4 forms of both weight-stream kernels (csrc/gemv_bf16.hip) reading every nibble value at
every position back exactly, exactly on integer operands and against float64 on random ones, the engine loaded from synthetic AWQ and GPTQ checkpoints
(as dicts and from disk) and get_embed on such an engine, against the oracle run on the dequantised weights W^.

Random-operand bound (linear_tol, the 8-bit and MXFP4 tests' bound): the kernels form exact products (bf16 x W^, both bf16 values) and add them in fp32 in
some order, then round once: |y - ref| <= ulp_bf16(ref) + K 2^-24 sum_k |x_k w^_k|.  Every further rounding point of an epilogue adds its own ulp, carried
to the output.  The SAME bound is applied to the bf16 kernels on W^ at the same shape: a wrong bound fails there too.

No test knows the order of the nibbles in the library's packed bytes: packed tensors come out of repack_int4 only.
"""
import json
import re

import pytest
import torch

import qwen2_int4_common as C
from oracle import qwen2vl_ref as Q

pytestmark = pytest.mark.gpu

M_LIST = (1, 3, 4, 5, 16, 17, 33, 64)      # dot form <1>; matrix-core form MB = 1 (from 3 rows on, where the shape lets it), 1, 1, 1, 2, 3, 4
LAYOUTS = {"awq": C.LAYOUT_AWQ, "gptq": C.LAYOUT_GPTQ, "gptq_v2": C.LAYOUT_GPTQ_V2}


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def _repack(hip, layout, q, z, s, G):
    """(q, z, s) -> the library's (packed, scales, zeros) on the device, through the checkpoint layout and td_repack_int4."""
    t = {k: v.cuda() for k, v in C.pack(layout, q, z, s).items()}
    return hip.repack_int4(layout, t["qweight"], t["qzeros"], t["scales"], G, g_idx=t.get("g_idx"))


# ---- 1. repack + dequantise --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("N,K,G", [(8, 32, 32), (24, 256, 64), (64, 1536, 128), (40, 8960, 128)])
def test_repack_and_dequant_are_bit_exact(hip, layout, N, K, G):
    """All 256 (q, z) pairs (the 8 x 32 matrix has 8 groups: 128 of them) under fp16 subnormal, largest, negative and power-of-two scales: the device layout
    out of either checkpoint layout dequantises to the restatement's W^, and scales and zeros arrive transposed, unchanged."""
    q, z, s = C.edge_problem(N, K, G, seed=N + K)
    pairs = {(int(a), int(b)) for a, b in zip(q.flatten().tolist(), z.repeat_interleave(G, dim=1).flatten().tolist())}
    assert len(pairs) == min(256, 16 * N * (K // G))
    assert {2.0 ** -24, 65504.0, -65504.0, -1.0, 0.5, 2.0} <= set(s.flatten().tolist()[:8])
    ref = C.w_hat(q, z, s, G)
    packed, sc, zp = _repack(hip, LAYOUTS[layout], q, z, s, G)
    torch.cuda.synchronize()
    assert packed.shape == (N, K // 2) and packed.dtype == torch.uint8 and sc.dtype == torch.float16 and zp.dtype == torch.uint8
    assert torch.equal(sc.cpu().view(torch.int16), s.view(torch.int16)) and torch.equal(zp.cpu(), z)
    wh = hip.dequant_rows_int4(packed, sc, zp, G)
    torch.cuda.synchronize()
    assert torch.equal(wh.cpu(), ref), f"{int((wh.cpu() != ref).sum())} weights differ from the restatement"
    # into a strided view, and through the torch ops
    wide = torch.full((N, K + 64), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.dequant_rows_int4(packed, sc, zp, G, out=wide[:, :K])
    assert torch.equal(wide[:, :K], wh) and bool((wide[:, K:] == 7.0).all())
    import thinkdiff.ops  # noqa: F401
    t = {k: v.cuda() for k, v in C.pack(LAYOUTS[layout], q, z, s).items()}
    po, so, zo = torch.ops.thinkdiff_hip.repack_int4(LAYOUTS[layout], t["qweight"], t["qzeros"], t["scales"], G)
    assert torch.equal(po, packed) and torch.equal(so, sc) and torch.equal(zo, zp)
    assert torch.equal(torch.ops.thinkdiff_hip.dequant_rows_int4(packed, sc, zp, G), wh)


# ---- 2. every nibble value at every position ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [128, 32])
@pytest.mark.parametrize("N", [16, 20])
def test_linear_i4_reads_every_nibble_back(hip, N, G):
    """A weight [N, 512] in which every k holds all 16 nibble values down the rows, zero points that change with row and group, and scales from the edge
    set: one-hot activation rows read every W^[n, k] back exactly.  N = 16: the dot form (M <= 2) and the matrix-core form (M > 2: K % 256 == 0,
    N % 16 == 0); N = 20, which the matrix core does not take: the dot forms <1>, <4>, <4>, <8>, <16> (more than 16 rows have no kernel there).  Pins
    nibble order, zero point, scale and group placement in every kernel form."""
    K, N8 = 512, (N + 7) // 8 * 8      # (a checkpoint packs 8 output rows into a word: N = 20 is the first 20 rows of a 24-row Linear)
    n, k = torch.arange(N8)[:, None], torch.arange(K)[None, :]
    q = ((k + 5 * n) % 16).to(torch.uint8)
    assert all(sorted(set(q[:16, kk].tolist())) == list(range(16)) for kk in range(K))
    z = ((torch.arange(K // G)[None, :] * 3 + n) % 16).to(torch.uint8)
    s = torch.tensor([0.5, -1.0, 2.0 ** -24, 65504.0, -0.0072021484375, 3.0], dtype=torch.float32).half()[(2 * n + torch.arange(K // G)[None, :]) % 6]
    w_hat = C.w_hat(q, z, s, G)[:N]
    packed, sc, zp = (t[:N] for t in _repack(hip, C.LAYOUT_AWQ, q, z, s, G))
    assert torch.equal(hip.dequant_rows_int4(packed, sc, zp, G).cpu(), w_hat)
    eye = torch.eye(K, dtype=torch.bfloat16, device="cuda")
    want = w_hat.float().T.contiguous()
    for M in [m for m in M_LIST if N % 16 == 0 or m <= 16]:
        starts = list(range(0, K - M + 1, M)) + ([K - M] if K % M else [])
        ys = [hip.linear_i4(eye[s0:s0 + M], packed, sc, zp, G) for s0 in starts]
        torch.cuda.synchronize()
        got = torch.empty(K, N)
        for s0, y in zip(starts, ys):
            got[s0:s0 + M] = y.float().cpu()
        assert torch.equal(got, want), f"M={M}: {int((got != want).sum())} weights are not read back as W^"


# ---- 3. exact integers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 8960), (48, 512)])
def test_linear_i4_exact_integers(hip, N, K):
    """Scales in {0.5, 1, 2} make W^ = (q - z) s multiples of a half below 32, and x small integers: every product and every partial sum is exact in fp32
    (and in float64), so the output is bf16(float64) bit for bit whatever the order of the sum."""
    G = 128
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    q = ((3 * n + 5 * k + (n * k) % 7) % 16).to(torch.uint8)
    z = ((n + 2 * torch.arange(K // G)[None, :]) % 16).to(torch.uint8)
    s = torch.tensor([0.5, 1.0, 2.0]).half()[(n + torch.arange(K // G)[None, :]) % 3]
    w = C.w_hat(q, z, s, G)
    assert torch.equal(w.double(), (q.double() - z.double().repeat_interleave(G, dim=1)) * s.double().repeat_interleave(G, dim=1))
    packed, sc, zp = _repack(hip, C.LAYOUT_GPTQ, q, z, s, G)
    for M in M_LIST:
        m = torch.arange(M)[:, None]
        x = ((2 * m + 3 * k + (m * k) % 5) % 9 - 4).float()
        ref = (x.double() @ w.double().T).float().bfloat16()           # bf16(float64 result): the float64 sum is exact too
        y = hip.linear_i4(x.bfloat16().cuda(), packed, sc, zp, G)
        torch.cuda.synchronize()
        assert torch.equal(y.cpu(), ref), f"M={M}: {int((y.cpu() != ref).sum())} elements differ"


# ---- 4. random operands vs float64 on (x, W^) ----------------------------------------------------------------------------------------------
_WEIGHTS = {}


def _rand_weight(hip, N, K, G):
    """Random int4 weights made where they are used: uniform random int32 words in a checkpoint layout (AWQ or GPTQ by the parity of N / 8) and scales of
    magnitude 2^-9 .. 2^-6 through repack_int4; W^ from dequant_rows_int4, which test 1 holds to the restatement.  Made once per extent and shared,
    unchanged, by the cases of that extent (only the last one is kept: the large extents are a quarter of a GiB as bf16)."""
    if (N, K, G) not in _WEIGHTS:
        _WEIGHTS.clear()
        g = torch.Generator(device="cuda").manual_seed(1000003 * N + K + G)
        awq = (N // 8) % 2 == 1
        words = lambda *shape: (torch.randint(0, 2 ** 32, shape, generator=g, device="cuda") - 2 ** 31).to(torch.int32)      # noqa: E731  (all 32 bits random)
        qw, qz = words(K, N // 8) if awq else words(K // 8, N), words(K // G, N // 8)
        s = ((torch.rand(K // G, N, generator=g, device="cuda") + 1.0) * 2.0 ** -9 * (torch.randint(0, 2, (K // G, N), generator=g, device="cuda") * 2 - 1)).half()
        p, sc, zp = hip.repack_int4(C.LAYOUT_AWQ if awq else C.LAYOUT_GPTQ, qw, qz, s, G)
        _WEIGHTS[(N, K, G)] = (p, sc, zp, hip.dequant_rows_int4(p, sc, zp, G))
    return _WEIGHTS[(N, K, G)]


def _rand_problem(hip, M, N, K, G, seed):
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).bfloat16()
    return (x.cuda(),) + _rand_weight(hip, N, K, G)


def _dots(x, wh):
    """float64 x . W^T and sum_k |x_k w^_k| (on the device: torch's float64 matmul)."""
    xd, wd = x.double(), wh.double()
    return xd @ wd.T, xd.abs() @ wd.abs().T


def _check(got, ref, tol, what):
    err = (got.double() - ref).abs()
    worst = float((err / tol).max())
    print(f"{what}: max error {worst:.3f} x the bound")
    assert worst <= 1.0, f"{what}: {int((err > tol).sum())} / {err.numel()} elements beyond the bound (worst {worst:.3f} x)"


def _r16(t):
    return t.bfloat16().double()


# The int4 routing is the MXFP4 routing (td_gemv_launch: up to 2 rows the dot form, more on the matrix core where the shape lets it; a k-step is 256
# weights in both), so the shapes that reach every instantiation are those of tests/test_qwen2_w4_gpu.py's PLAIN
PLAIN = [  # (M, N, K, G, what runs)
    (1, 64, 8960, 128, "dot form <1>: main loop and tail"),
    (2, 64, 8960, 128, "dot form <2>: main loop and tail"),
    (2, 64, 8960, 32, "dot form <2>, G = 32: main loop and tail"),
    (4, 40, 8960, 128, "dot form <4> (N % 16 != 0; the matrix core takes 3 .. 4 rows where it can): main loop and tail"),
    (4, 64, 8960, 128, "MFMA <1, 1, shallow> with K split over 4 workgroups: 3 .. 4 rows go to the matrix core"),
    (3, 64, 128, 128, "dot form <4>: K too short for the main loop"),
    (8, 40, 192, 64, "dot form <8>: 5 .. 8 rows of a shape the matrix core does not take (K % 256, N % 16), K too short for the main loop, G = 64"),
    (13, 40, 192, 32, "dot form <16>, K too short for the main loop, G = 32"),
    (8, 40, 8960, 128, "dot form <8> (N % 16 != 0): main loop and tail"),
    (13, 40, 8960, 128, "dot form <16> (N % 16 != 0): main loop and tail"),
    # the matrix-core form <MB, NR, DEEP>: MB = ceil(M / 16); NR = 2 from 1024 weight blocks (N >= 16384) on, for MB > 1; DEEP when a workgroup
    # has at least 32 of the 256-element steps (K / 256 / ks, ks = K parts = min(8, 512 / blocks, steps / 8) below 256 blocks): all 14 forms
    (5, 64, 4096, 128, "MFMA <1, 1, shallow> with K split over 2 workgroups"),
    (5, 64, 4096, 32, "MFMA <1, 1, shallow> with K split over 2 workgroups, G = 32"),
    (17, 64, 4096, 64, "MFMA <2, 1, shallow>, K split over 2 workgroups, G = 64"),
    (16, 4096, 8192, 128, "MFMA <1, 1, DEEP>"),
    (17, 4096, 8192, 128, "MFMA <2, 1, DEEP>"),
    (48, 256, 1024, 128, "MFMA <3, 1, shallow>: 4 steps, half the waves idle"),
    (48, 3584, 16384, 128, "MFMA <3, 1, DEEP> with K split over 2 workgroups (the 7B down_proj's form: 224 blocks)"),
    (64, 3584, 16384, 128, "MFMA <4, 1, DEEP> with K split over 2 workgroups"),
    (64, 320, 512, 128, "MFMA <4, 1, shallow>"),
    (64, 64, 8960, 128, "MFMA <4, 1, shallow> with K split over 4 workgroups (35 steps)"),
    (17, 16384, 256, 128, "MFMA <2, 2, shallow>: two weight blocks per workgroup, one step"),
    (48, 16384, 256, 128, "MFMA <3, 2, shallow>"),
    (64, 16384, 256, 128, "MFMA <4, 2, shallow>"),
    (17, 16384, 8192, 128, "MFMA <2, 2, DEEP>"),
    (33, 16384, 8192, 128, "MFMA <3, 2, DEEP>"),
    (64, 16384, 8192, 32, "MFMA <4, 2, DEEP>, G = 32"),
]


@pytest.mark.parametrize("M,N,K,G,what", PLAIN, ids=[f"{m}x{n}x{k}-g{g}-" + re.match(r"dot form <\d+>|MFMA <[^>]*>", w).group(0).replace(" ", "") for m, n, k, g, w in PLAIN])
def test_linear_i4_random_vs_float64(hip, M, N, K, G, what):
    """Plain Linear at shapes that make td_gemv_launch pick every int4 instantiation of both kernels: the dot form <1, 2, 4, 8, 16> and all 14
    <MB, NR, DEEP> forms of the matrix-core kernel (PLAIN names the form each shape runs); the torch op on one of them."""
    x, p, sc, zp, wh = _rand_problem(hip, M, N, K, G, seed=M * 131 + N + K)
    ref, absdot = _dots(x, wh)
    tol = C.linear_tol(ref, absdot, K)
    y4 = hip.linear_i4(x, p, sc, zp, G)
    y16 = hip.linear(x, wh)
    torch.cuda.synchronize()
    _check(y4, ref, tol, f"i4 {what}")
    _check(y16, ref, tol, f"bf16 on W^, {M}x{N}x{K}")
    if (M, N, K, G) == (5, 64, 4096, 128):
        import thinkdiff.ops  # noqa: F401
        assert torch.equal(torch.ops.thinkdiff_hip.linear_i4(x, p, sc, zp, G, None, 0, None, None), y4)


# ---- 5. epilogues ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(4, 64, 1536), (33, 64, 2048)])
def test_linear_i4_bias_act_residual(hip, M, N, K):
    """y = bf16(bf16(silu(bf16(acc + bias))) + res): the Linear output rounds, the activation rounds, the residual sum rounds.  silu has slope <= 1.1
    and is evaluated in fp32 with v_exp / v_rcp (<= 2^-20 relative, generous).  M = 4: MFMA <1, 1>; M = 33: MFMA <3, 1>.  The MXFP4 test's bounds."""
    G = 128
    x, p, sc, zp, wh = _rand_problem(hip, M, N, K, G, seed=M + K)
    g = torch.Generator().manual_seed(7)
    bias = torch.randn(N, generator=g).bfloat16().cuda()
    res = torch.randn(M, N, generator=g).bfloat16().cuda()
    dot, absdot = _dots(x, wh)
    inner = dot + bias.double()
    ref = _r16(inner) + res.double()
    tol = C.ulp_bf16(ref) + C.ulp_bf16(inner) + C.sum_bound(K, absdot)
    y4 = hip.linear_i4(x, p, sc, zp, G, bias=bias, res=res)
    y16 = hip.linear(x, wh, bias=bias, res=res)
    torch.cuda.synchronize()
    _check(y4, ref, tol, "i4 bias + residual")
    _check(y16, ref, tol, "bf16 bias + residual")
    # the residual may be the output itself (the engine's h += ...)
    out = res.clone()
    hip.linear_i4(x, p, sc, zp, G, bias=bias, res=out, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, y4)
    # ... with SiLU between the Linear and the residual
    i16 = _r16(inner)
    a_ref = i16 * torch.sigmoid(i16)
    ref = _r16(a_ref) + res.double()
    d_in = C.sum_bound(K, absdot) + C.ulp_bf16(inner)
    d_act = 1.1 * d_in + 2.0 ** -20 * a_ref.abs() + C.ulp_bf16(a_ref)
    tol = C.ulp_bf16(ref) + d_act
    y4 = hip.linear_i4(x, p, sc, zp, G, bias=bias, act=hip.ACT_SILU, res=res)
    y16 = hip.linear(x, wh, bias=bias, act=hip.ACT_SILU, res=res)
    torch.cuda.synchronize()
    _check(y4, ref, tol, "i4 bias + silu + residual")
    _check(y16, ref, tol, "bf16 bias + silu + residual")


@pytest.mark.parametrize("M,N,K,n_split", [(1, 96, 1536, 64), (48, 96, 1024, 64)])
def test_linear_i4_split_output(hip, M, N, K, n_split):
    """Columns < n_split to one buffer, the rest to another (the q | k|v projection's form), with bias: no further rounding point."""
    G = 128
    x, p, sc, zp, wh = _rand_problem(hip, M, N, K, G, seed=M + N)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(5)).bfloat16().cuda()
    dot, absdot = _dots(x, wh)
    ref = dot + bias.double()
    tol = C.linear_tol(ref, absdot, K)
    for fn, args, what in ((hip.linear_split_i4, (x, p, sc, zp, G), "i4"), (hip.linear_split, (x, wh), "bf16")):
        y0 = torch.zeros(M, n_split, dtype=torch.bfloat16, device="cuda")
        y1 = torch.zeros(M, N - n_split, dtype=torch.bfloat16, device="cuda")
        fn(*args, bias, y0, 0, y1, 0, n_split)
        torch.cuda.synchronize()
        _check(torch.cat([y0, y1], dim=1), ref, tol, f"{what} split output")


@pytest.mark.parametrize("M,inter,K,G", [(2, 64, 1536, 128), (8, 40, 96, 32), (17, 64, 1024, 128), (33, 2048, 4096, 128), (5, 64, 2048, 128)])
def test_linear_i4_glu(hip, M, inter, K, G):
    """out = bf16(bf16(silu(bf16(g))) * bf16(u)), g / u = x . gate / up rows, at the MXFP4 test's shapes (K = 96 takes G = 32) and with its bound, carried
    through the chain: dg = sum bound + ulp(g); ds = 1.1 dg + 2^-20 |s| + ulp(s); du = sum bound + ulp(u); product: |s| du + |u| ds + ds du; plus the
    output's ulp."""
    x, p, sc, zp, wh = _rand_problem(hip, M, 2 * inter, K, G, seed=M + inter)
    dot, absdot = _dots(x, wh)
    gd, ud = dot[:, :inter], dot[:, inter:]
    g16, u16 = _r16(gd), _r16(ud)
    s_ref = g16 * torch.sigmoid(g16)
    s16 = _r16(s_ref)
    ref = s16 * u16
    dg = C.sum_bound(K, absdot[:, :inter]) + C.ulp_bf16(gd)
    ds = 1.1 * dg + 2.0 ** -20 * s_ref.abs() + C.ulp_bf16(s_ref)
    du = C.sum_bound(K, absdot[:, inter:]) + C.ulp_bf16(ud)
    tol = C.ulp_bf16(ref) + s16.abs() * du + u16.abs() * ds + ds * du
    y4 = hip.linear_glu_i4(x, p, sc, zp, G)
    y16 = hip.linear_glu(x, wh)
    torch.cuda.synchronize()
    _check(y4, ref, tol, "i4 gated")
    _check(y16, ref, tol, "bf16 gated")


# ---- 6. the engine ---------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"awq": {"quant_method": "awq", "bits": 4, "group_size": 128, "version": "gemm", "zero_point": True},
           "gptq": {"quant_method": "gptq", "bits": 4, "group_size": 128, "desc_act": False, "sym": False}}


def _engine(cfg, sd, max_len, int4_config=None, quantization=None):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    e = Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                                            num_key_value_heads=cfg.num_kv_heads, intermediate_size=cfg.intermediate, vocab_size=cfg.vocab,
                                            tie_word_embeddings=cfg.tie_embeddings), max_model_len=max_len)
    e.weight_quantization = quantization
    e.int4_config = int4_config
    if sd is not None:
        e.load_state_dict(sd)
    return e


def _int4_bytes(cfg, G):
    D, I, NQKV = cfg.hidden, cfg.intermediate, (cfg.num_heads + 2 * cfg.num_kv_heads) * 128
    elems = cfg.num_layers * (NQKV * D + D * cfg.num_heads * 128 + 2 * I * D + D * I)
    return elems // 2 + 3 * elems // G


@pytest.mark.parametrize("method,tie", [("awq", False), ("awq", True), ("gptq", False), ("gptq", True)])
def test_engine_decode_with_int4_weights(hip, method, tie):
    cfg = Q.tiny_config(tie_embeddings=tie)
    sd = Q.init_weights(cfg, seed=41 + int(tie))
    G = 128
    ck, sd_hat = C.int4_state_dict(sd, C.LAYOUT_AWQ if method == "awq" else C.LAYOUT_GPTQ, G, seed=5)
    n0, BMAX, SLOTS = 40, 64, 66
    e = _engine(cfg, ck, max_len=SLOTS * 128, int4_config=CONFIGS[method])
    assert e.weight_info() == {"mode": "int4", "stream_on": True, "bytes_8bit": _int4_bytes(cfg, G), "n_linears": 7 * cfg.num_layers}
    e.set_slots(SLOTS)
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, cfg.vocab, (n0,), generator=g).to(torch.int32)
    toks = torch.randperm(cfg.vocab, generator=g)[:SLOTS].to(torch.int32)
    pos = Q.text_position_ids(n0)
    hid_p, _ = e.forward(pos, prompt, slot=0)
    for b in range(1, SLOTS):
        e.move_slot(0, b, n0)
    # the oracle on W^: the prompt once (its k / v are the cache), then every sequence's next token
    ref16, ref32, lref = [], [], []
    sd32 = {k: v.float() for k, v in sd_hat.items()}
    p16, kv16 = Q.text_model_hidden(sd_hat, cfg, pos, token_ids=prompt.long())
    _, kv32 = Q.text_model_hidden(sd32, cfg, pos, token_ids=prompt.long())
    assert _rel(hid_p, p16) < 2e-2
    pos1 = Q.text_position_ids(1, start=n0)
    for b in range(BMAX):
        h16, _ = Q.text_model_hidden(sd_hat, cfg, pos1, token_ids=toks[b:b + 1].long(), past=kv16)
        h32, _ = Q.text_model_hidden(sd32, cfg, pos1, token_ids=toks[b:b + 1].long(), past=kv32)
        ref16.append(h16[-1])
        ref32.append(h32[-1])
        lref.append(Q.lm_logits(sd_hat, cfg, h16[-1]))
    ref16, ref32, lref = torch.stack(ref16), torch.stack(ref32), torch.stack(lref)

    def step(B):
        outs = [e.decode_batch(toks[:B], torch.full((3, B), n0, dtype=torch.int32), [n0] * B) for _ in range(3)]   # eager, captured, replayed
        torch.cuda.synchronize()
        for h, lg in outs[1:]:
            assert torch.equal(h, outs[0][0]) and torch.equal(lg, outs[0][1])
        return outs[0][0].clone(), outs[0][1].clone()

    # the handle counts the launches that read the copy: step() is 3 calls = an eager step and a captured one (2 x 4 Linears per layer; lm_head has no
    # copy and reads bf16) and a replay, which counts nothing.  By default only the row counts at which the int4 forms measured faster than bf16 are routed
    # to them: at this width (hidden < 3072) 17 .. 64 rows, the others read the bf16 arena with the stream on too.  set_int4_routing(True)
    # sends every row count to them: the dot form at 1 and 2 rows and the matrix-core form MB = 1 .. 4 through the engine's fused q|k|v (split output),
    # gated and residual launches
    per_step = 4 * cfg.num_layers
    assert e.set_int4_routing(True) is False
    for B, routed in ((1, True), (2, True), (3, True), (5, True), (17, True), (33, True), (64, True), (1, False), (3, False), (16, False), (17, True), (64, True)):
        if not routed:
            e.set_int4_routing(False)
        assert e.set_weight_stream(True) in (True, False)
        n_before = e.weight_stream_launches()
        on_h, on_l = step(B)
        n_on = e.weight_stream_launches() - n_before
        if routed:
            assert n_on in (2 * per_step, 3 * per_step), f"the decode step read the int4 copy in {n_on} launches"     # (3 x: a runtime that cannot capture)
        else:
            assert n_on == 0, f"a step of {B} sequences is not routed to the int4 forms at this width, yet {n_on} launches read the copy"
        assert e.set_weight_stream(False) is True
        off_h, off_l = step(B)
        assert e.weight_stream_launches() - n_before == n_on, "stream off still read the int4 copy"
        e.set_weight_stream(True)
        eref = _rel(ref16[:B], ref32[:B])
        for name, h, lg in (("stream on", on_h, on_l), ("stream off", off_h, off_l)):
            e16, e32 = _rel(h, ref16[:B]), _rel(h, ref32[:B])
            print(f"B={B} {name}: rel-RMSE hip~bf16 {e16:.4f} hip~fp32 {e32:.4f} bf16~fp32 {eref:.4f}")
            assert e16 < 2e-2 and e32 < 1.5 * eref + 2e-3
            assert _rel(lg, lref[:B]) < 3e-2
        assert _rel(on_h, off_h) < 2e-2 and _rel(on_h, ref32[:B]) < 1.5 * _rel(off_h, ref32[:B]) + 2e-3
        assert _rel(on_l, off_l) < 3e-2

    assert e.set_int4_routing(True) is False and e.set_int4_routing(False) is True
    # more than 64 rows never read the int4 copy: identical bits with the stream on and off
    wide = {}
    n_before = e.weight_stream_launches()
    for on in (True, False):
        e.set_weight_stream(on)
        wide[on] = step(65)
    for a, b in zip(wide[True], wide[False]):
        assert torch.equal(a, b)
    assert e.weight_stream_launches() == n_before
    e.set_weight_stream(True)

    # the bf16 weights the engine holds ARE the restatement's W^: with the stream off (every Linear reads the arena) prefill and decode equal, bit for
    # bit, a bf16 engine loaded with the restatement's values
    plain = _engine(cfg, sd_hat, max_len=SLOTS * 128)
    plain.set_slots(SLOTS)
    e.set_weight_stream(False)
    both = []
    for eng in (e, plain):
        h = eng.forward(pos, prompt, slot=0)[0].clone()
        for b in (1, 2):
            eng.move_slot(0, b, n0)
        d = eng.decode_batch(toks[:3], torch.full((3, 3), n0, dtype=torch.int32), [n0] * 3)
        torch.cuda.synchronize()
        both.append((h, d[0].clone(), d[1].clone()))
    for a, b in zip(*both):
        assert torch.equal(a, b), "the arena of the int4 engine is not the restatement's W^"
    e.set_weight_stream(True)
    e.forward(pos, prompt, slot=0)
    for b in range(1, SLOTS):
        e.move_slot(0, b, n0)
    before = step(17)

    # loading the checkpoint again leaves the handle whole and the output bit-equal; biases, norms, embeddings and lm_head load as ever
    e.load_state_dict(ck)
    e.load_state_dict({k: v for k, v in sd.items() if k.endswith(".bias") or "norm" in k or "embed" in k or k.startswith("lm_head")}, strict=False)
    again = step(17)
    assert torch.equal(before[0], again[0]) and torch.equal(before[1], again[1])

    # mixing modes is refused, each message naming the rule
    with pytest.raises(hip.ThinkDiffHipError, match="TD_QWEN2_WEIGHTS_INT4.*one weight format"):
        e.quantize_weights("mxfp4")
    with pytest.raises(hip.ThinkDiffHipError, match="TD_QWEN2_WEIGHTS_INT4.*one weight format"):
        e.quantize_weights("fp8")
    name = "model.layers.1.mlp.down_proj.weight"
    with pytest.raises(hip.ThinkDiffHipError, match="down_proj.weight.*TD_QWEN2_WEIGHTS_INT4.*one weight format"):
        e.load_state_dict({name: sd[name]}, strict=False)
    with pytest.raises(hip.ThinkDiffHipError, match="td_qwen2_init_random.*TD_QWEN2_WEIGHTS_INT4.*one weight format"):
        e.init_random(seed=1)
    ck64, _ = C.int4_state_dict({name: sd[name]}, C.LAYOUT_AWQ if method == "awq" else C.LAYOUT_GPTQ, 64, seed=9)
    e.int4_config = {**CONFIGS[method], "group_size": 64}
    with pytest.raises(hip.ThinkDiffHipError, match="G=64.*group size 128.*one group size"):
        e.load_state_dict(ck64, strict=False)
    e.int4_config = CONFIGS[method]
    assert e.weight_info()["mode"] == "int4"
    again = step(17)
    assert torch.equal(before[0], again[0]) and torch.equal(before[1], again[1])


def test_int4_mode_mixing_on_other_handles(hip):
    cfg = Q.tiny_config()
    sd = Q.init_weights(cfg, seed=5)
    ck, _ = C.int4_state_dict(sd, C.LAYOUT_AWQ, 128, seed=1)
    prompt = torch.arange(7, 27, dtype=torch.int32)
    # an E4M3 / MXFP4 handle refuses int4 Linears, naming its mode
    for q, mode in (("fp8", "TD_QWEN2_WEIGHTS_E4M3"), ("mxfp4", "TD_QWEN2_WEIGHTS_MXFP4")):
        e = _engine(cfg, sd, max_len=128, quantization=q)
        with pytest.raises(hip.ThinkDiffHipError, match="td_qwen2_set_int4_routing.*no int4 weights"):
            e.set_int4_routing(True)
        e.weight_quantization, e.int4_config = None, CONFIGS["awq"]      # (past the loader's own refusal, which test_qwen2_int4_cpu.py covers)
        with pytest.raises(hip.ThinkDiffHipError, match="td_qwen2_load_param_int4.*" + mode + ".*one weight format"):
            e.load_state_dict(ck)
        assert e.weight_info()["mode"] == q
    # a handle with int4 data for some of its Linears refuses every run, naming the entry that completes it
    e = _engine(cfg, None, max_len=128, int4_config=CONFIGS["awq"])
    some = {k: v for k, v in ck.items() if "layers.0." in k}
    e.load_state_dict(some, strict=False)
    assert e.weight_info()["mode"] == "int4" and e.weight_info()["stream_on"] is False
    with pytest.raises(hip.ThinkDiffHipError, match="7 of its 14 decoder Linears.*td_qwen2_load_param_int4"):
        e.forward(Q.text_position_ids(20), prompt, slot=0)
    e.load_state_dict(ck)
    assert e.weight_info()["stream_on"] is True
    e.forward(Q.text_position_ids(20), prompt, slot=0)
    torch.cuda.synchronize()
    # int4 tensors on an engine told to quantise: the loader's refusal, before any device work
    with pytest.raises(ValueError, match="weight_quantization='mxfp4'"):
        _engine(cfg, ck, max_len=128, int4_config=CONFIGS["awq"], quantization="mxfp4")


# ---- 7. load_pretrained ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["awq", "gptq"])
def test_load_pretrained_detects_and_loads_int4(hip, tmp_path, method):
    """A checkpoint directory -- two safetensors shards that split the tensors of one Linear between them, plus a config.json with the checkpoint's
    quantization_config -- loads as int4 with nothing set on the engine, into the state the dict route gives."""
    from safetensors.torch import save_file
    cfg = Q.tiny_config()
    sd = Q.init_weights(cfg, seed=12)
    ck, _ = C.int4_state_dict(sd, C.LAYOUT_AWQ if method == "awq" else C.LAYOUT_GPTQ, 128, seed=3)
    keys = sorted(ck)
    cut = keys.index("model.layers.0.mlp.up_proj.qzeros")        # (qweight | qzeros, scales of that Linear fall into different shards)
    save_file({k: ck[k].contiguous() for k in keys[:cut]}, str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file({**{k: ck[k].contiguous() for k in keys[cut:]}, "visual.blocks.0.attn.qkv.weight": torch.zeros(8, 8)}, str(tmp_path / "model-00002-of-00002.safetensors"))
    with open(tmp_path / "config.json", "w") as fh:
        json.dump({"model_type": "qwen2_vl", "quantization_config": CONFIGS[method]}, fh)
    disk = _engine(cfg, None, max_len=128)
    assert disk.int4_config is None
    disk.load_pretrained(str(tmp_path))
    assert disk.int4_config == CONFIGS[method]
    mem = _engine(cfg, ck, max_len=128, int4_config=CONFIGS[method])
    assert disk.weight_info() == mem.weight_info() and disk.weight_info()["mode"] == "int4" and disk.weight_info()["stream_on"]
    prompt = torch.randint(0, cfg.vocab, (24,), generator=torch.Generator().manual_seed(1)).to(torch.int32)
    outs = []
    for e in (disk, mem):
        h, _ = e.forward(Q.text_position_ids(24), prompt, slot=0)
        d = e.decode_batch(torch.tensor([5], dtype=torch.int32), torch.full((3, 1), 24, dtype=torch.int32), [24])
        torch.cuda.synchronize()
        outs.append((h.clone(), d[0].clone(), d[1].clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- 8. get_embed ----------------------------------------------------------------------------------------------------------------------------
def test_get_embed_with_int4_checkpoint(hip):
    """ThinkDiff-LVLM get_embed, teacher-forced as tests/test_qwen2_gpu.py::test_get_embed_teacher_forced, on an engine loaded from a synthetic AWQ
    checkpoint: the aligner restatement on the oracle run on W^, within that test's 3e-2."""
    from oracle import aligner_ref as A
    from thinkdiff.models.mllama_vllm_t5_embed_decoder_2 import MllamaVllmT5EmbedDecoderForConditionalGeneration_5
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig
    cfg = Q.tiny_config()
    sd = Q.init_weights(cfg, seed=9)
    ck, sd_hat = C.int4_state_dict(sd, C.LAYOUT_AWQ, 128, seed=2)
    asd = A.init_weights(cfg.hidden, 4096, seed=4)
    tc = Qwen2VLTextConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                           num_key_value_heads=cfg.num_kv_heads, intermediate_size=cfg.intermediate, vocab_size=cfg.vocab)
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, cfg.vocab, (20,), generator=g).tolist()
    forced = torch.randint(0, cfg.vocab, (6,), generator=g).tolist()

    def ref_aligner(h):
        F = torch.nn.functional
        y = F.linear(F.gelu(F.linear(h, asd["mm_projector.0.weight"], asd["mm_projector.0.bias"])), asd["mm_projector.2.weight"], asd["mm_projector.2.bias"])
        return A.t5_layer_norm(y.float(), asd["mm_projector.3.weight"].float()).bfloat16()

    m = MllamaVllmT5EmbedDecoderForConditionalGeneration_5(tc, vllm_config={"max_model_len": 256, "max_tokens": 6, "min_tokens": 6})
    m.mllama.int4_config = CONFIGS["awq"]
    m.mllama.load_state_dict(ck)
    m.load_state_dict(asd)
    assert m.mllama.weight_info()["mode"] == "int4" and m.mllama.weight_info()["stream_on"]
    ref_h, _ = Q.text_model_hidden(sd_hat, cfg, Q.text_position_ids(26), token_ids=torch.tensor(prompt + forced))
    for et, sl in [("both", slice(0, 26)), ("output_embed", slice(20, 26))]:
        embs, texts = m.get_embed([{"prompt_token_ids": prompt}], embedding_type=et, need_process=False, forced_output_ids=[forced])
        torch.cuda.synchronize()
        assert texts == [" ".join(map(str, forced))]
        assert embs[0].shape == (sl.stop - sl.start, 4096)
        assert _rel(embs[0], ref_aligner(ref_h[sl])) < 3e-2
