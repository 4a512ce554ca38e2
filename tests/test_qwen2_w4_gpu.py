"""The MXFP4 weight stream of the Qwen2-VL decode engine on the GPU: the quantiser bit for bit against the CPU restatement
(tests/qwen2_w4_common.py), the 4-bit forms of both weight-stream kernels (csrc/gemv_bf16.hip) reading every byte value under three scales back
exactly, exactly on integer operands and against float64 on random ones, the engine / the pre-quantised loader / get_embed with MXFP4 weights against
the oracle run on the dequantised weights W^.

Random-operand bound (linear_tol, the 8-bit tests' bound): the kernels form exact products (bf16 x W^, both bf16 values) and add them in fp32 in some
order, then round once: |y - ref| <= ulp_bf16(ref) + K 2^-24 sum_k |x_k w^_k|.  Every further rounding point of an epilogue adds its own ulp, carried to
the output.  The SAME bound is applied to the bf16 kernels on W^ at the same shape: a wrong bound fails there too.
"""
import pytest
import torch

import qwen2_w4_common as C
from oracle import qwen2vl_ref as Q

pytestmark = pytest.mark.gpu

M_LIST = (1, 3, 4, 5, 16, 17, 33, 64)      # dot form <1>; matrix-core form MB = 1 (from 3 rows on, where the shape lets it), 1, 1, 1, 2, 3, 4


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


# ---- 1. the quantiser ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 19, 64])
@pytest.mark.parametrize("K", [32, 1536, 8960])
def test_quantiser_is_bit_exact(hip, N, K):
    w = C.edge_blocks(N, K, seed=3 * N + K)
    p_ref, s_ref, wh_ref, _ = C.quantize_blocks(w)
    wd = w.cuda()
    p, s, wh = hip.quant_weight_rows_mxfp4(wd)
    torch.cuda.synchronize()
    assert torch.equal(s.cpu(), s_ref)
    assert torch.equal(p.cpu(), p_ref)
    assert torch.equal(C.bf16_bits(wh.cpu()), C.bf16_bits(wh_ref))    # the bits: -0 stays -0
    assert torch.equal(wd.cpu(), w)                                   # the input is untouched unless aliased
    assert torch.equal(hip.dequant_rows_mxfp4(p, s), wh)
    # no W^ wanted; W^ over the input (a strided view: the row stride is not K)
    p2, s2, none = hip.quant_weight_rows_mxfp4(wd, want_w_hat=False)
    assert none is None and torch.equal(p2, p) and torch.equal(s2, s)
    wide = torch.full((N, K + 64), 7.0, dtype=torch.bfloat16, device="cuda")
    wide[:, :K] = wd
    p3, s3, wh3 = hip.quant_weight_rows_mxfp4(wide[:, :K], inplace=True)
    torch.cuda.synchronize()
    assert wh3.data_ptr() == wide.data_ptr() and torch.equal(p3, p) and torch.equal(s3, s)
    assert torch.equal(C.bf16_bits(wide[:, :K].cpu()), C.bf16_bits(wh_ref)) and bool((wide[:, K:] == 7.0).all())
    # ... and the dequantiser into a strided view
    wide2 = torch.full((N, K + 64), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.dequant_rows_mxfp4(p, s, out=wide2[:, :K])
    assert torch.equal(wide2[:, :K], wh) and bool((wide2[:, K:] == 7.0).all())
    # quantising W^ gives the same bytes and W^
    p4, s4, wh4 = hip.quant_weight_rows_mxfp4(wh)
    assert torch.equal(wh4, wh) and torch.equal(p4, p)
    # the torch ops say the same
    import thinkdiff.ops  # noqa: F401
    po, so, who = torch.ops.thinkdiff_hip.quant_weight_rows_mxfp4(wd)
    assert torch.equal(po, p) and torch.equal(so, s) and torch.equal(who, wh)
    assert torch.equal(torch.ops.thinkdiff_hip.dequant_rows_mxfp4(p, s), wh)


# ---- 2. the decode table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 20])
def test_linear_w4_reads_every_byte_value_back(hip, N):
    """A weight [N, 512] whose packed bytes run through all 256 values in every row, under scale bytes 120, 127 and 134: one-hot activation rows read
    every W^[n, k] back exactly.  N = 16: the dot form (M <= 2) and the matrix-core form (M > 2: K % 256 == 0, N % 16 == 0); N = 20, which the matrix
    core does not take: the dot forms <1>, <4>, <4>, <8>, <16> (more than 16 rows have no kernel there).  Pins nibble order, sign, grid and scale
    placement in every kernel form."""
    K = 512
    n, j = torch.arange(N)[:, None], torch.arange(K // 2)[None, :]
    packed = ((j + 37 * n) % 256).to(torch.uint8)
    scales = torch.tensor([120, 127, 134], dtype=torch.uint8)[(n + torch.arange(K // 32)[None, :]) % 3]
    w_hat = C.dequantize(packed, scales)
    assert sorted(set(packed[3].tolist())) == list(range(256))
    pd, sd = packed.cuda(), scales.cuda()
    assert torch.equal(hip.dequant_rows_mxfp4(pd, sd).cpu().float(), w_hat)
    eye = torch.eye(K, dtype=torch.bfloat16, device="cuda")
    for M in [m for m in M_LIST if N % 16 == 0 or m <= 16]:
        starts = list(range(0, K - M + 1, M)) + ([K - M] if K % M else [])
        ys = [hip.linear_w4(eye[s0:s0 + M], pd, sd) for s0 in starts]
        torch.cuda.synchronize()
        got = torch.empty(K, N)
        for s0, y in zip(starts, ys):
            got[s0:s0 + M] = y.float().cpu()
        assert torch.equal(got, w_hat.T.contiguous()), f"M={M}: {int((got != w_hat.T).sum())} weights are not read back as the table says"


# ---- 3. exact integers -----------------------------------------------------------------------------------------------------------------------
def _int_problem(N, K):
    """Weights on the e2m1 grid (all 15 values) under block scales 1 and 2: the restatement reproduces W exactly and every fp32 sum of x W products is
    exact (integers and halves below 2^23)."""
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    code = (3 * n + 5 * k + (n * k) % 7) % 16
    blk_scale = 1.0 + ((n + k // 32) % 2).float()
    w = torch.tensor(C.TABLE)[code] * blk_scale
    w[:, 5::32] = 6.0 * blk_scale[:, 5::32]                      # every block holds a 6: its exponent is that of its scale
    p, s, wh, e = C.quantize_blocks(w)
    assert torch.equal(wh, w) and sorted(set(e.flatten().tolist())) == [0, 1]
    return w, p.cuda(), s.cuda()


@pytest.mark.parametrize("N,K", [(64, 8960), (48, 512)])
def test_linear_w4_exact_integers(hip, N, K):
    w, p, s = _int_problem(N, K)
    for M in M_LIST:
        m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
        x = ((2 * m + 3 * k + (m * k) % 5) % 9 - 4).float()
        ref = (x.double() @ w.double().T).float().bfloat16()           # bf16(float64 result): the float64 sum is exact too
        y = hip.linear_w4(x.bfloat16().cuda(), p, s)
        torch.cuda.synchronize()
        assert torch.equal(y.cpu(), ref), f"M={M}: {int((y.cpu() != ref).sum())} elements differ"


# ---- 4. random operands vs float64 on (x, W^) ----------------------------------------------------------------------------------------------
_WEIGHTS = {}


def _rand_weight(N, K):
    """Random MXFP4 weights made where they are used: uniform random bytes under block scales 2^-8 .. 2^-2, W^ from the restatement's table.  Made once
    per (N, K) and shared, unchanged, by the cases of that extent (only the last one is kept: the large extents are a quarter of a GiB as bf16)."""
    if (N, K) not in _WEIGHTS:
        _WEIGHTS.clear()
        g = torch.Generator(device="cuda").manual_seed(1000003 * N + K)
        p = torch.randint(0, 256, (N, K // 2), generator=g, device="cuda", dtype=torch.uint8)
        s = torch.randint(119, 126, (N, K // 32), generator=g, device="cuda", dtype=torch.uint8)
        _WEIGHTS[(N, K)] = (p, s, C.dequantize(p, s).bfloat16())
    return _WEIGHTS[(N, K)]


def _rand_problem(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).bfloat16()
    p, s, wh = _rand_weight(N, K)
    return x.cuda(), p, s, wh


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


PLAIN = [  # (M, N, K, what runs)
    (1, 64, 8960, "dot form <1>: main loop and tail"),
    (2, 64, 8960, "dot form <2>: main loop and tail"),
    (4, 40, 8960, "dot form <4> (N % 16 != 0; the matrix core takes 3 .. 4 rows where it can): main loop and tail"),
    (4, 64, 8960, "MFMA <1, 1, shallow> with K split over 4 workgroups: 3 .. 4 rows go to the matrix core"),
    (3, 64, 128, "dot form <4>: K too short for the main loop"),
    (8, 40, 192, "dot form <8>: 5 .. 8 rows of a shape the matrix core does not take (K % 256, N % 16), K too short for the main loop"),
    (13, 40, 192, "dot form <16>, K too short for the main loop"),
    (8, 40, 8960, "dot form <8> (N % 16 != 0): main loop and tail"),
    (13, 40, 8960, "dot form <16> (N % 16 != 0): main loop and tail"),
    # the matrix-core form <MB, NR, DEEP>: MB = ceil(M / 16); NR = 2 from 1024 weight blocks (N >= 16384) on, for MB > 1; DEEP when a workgroup
    # has at least 32 of the 256-element steps (K / 256 / ks, ks = K parts = min(8, 512 / blocks, steps / 8) below 256 blocks): all 14 forms
    (5, 64, 4096, "MFMA <1, 1, shallow> with K split over 2 workgroups"),
    (17, 64, 4096, "MFMA <2, 1, shallow>, K split over 2 workgroups"),
    (16, 4096, 8192, "MFMA <1, 1, DEEP>"),
    (17, 4096, 8192, "MFMA <2, 1, DEEP>"),
    (48, 256, 1024, "MFMA <3, 1, shallow>: 4 steps, half the waves idle"),
    (48, 3584, 16384, "MFMA <3, 1, DEEP> with K split over 2 workgroups (the 7B down_proj's form: 224 blocks)"),
    (64, 3584, 16384, "MFMA <4, 1, DEEP> with K split over 2 workgroups"),
    (64, 320, 512, "MFMA <4, 1, shallow>"),
    (64, 64, 8960, "MFMA <4, 1, shallow> with K split over 4 workgroups (35 steps)"),
    (17, 16384, 256, "MFMA <2, 2, shallow>: two weight blocks per workgroup, one step"),
    (48, 16384, 256, "MFMA <3, 2, shallow> (lm_head's form at 33 - 48 sequences)"),
    (64, 16384, 256, "MFMA <4, 2, shallow>"),
    (17, 16384, 8192, "MFMA <2, 2, DEEP>"),
    (33, 16384, 8192, "MFMA <3, 2, DEEP>"),
    (64, 16384, 8192, "MFMA <4, 2, DEEP>"),
]


@pytest.mark.parametrize("M,N,K,what", PLAIN, ids=[f"{m}x{n}x{k}" for m, n, k, _ in PLAIN])
def test_linear_w4_random_vs_float64(hip, M, N, K, what):
    """Plain Linear at shapes that make td_gemv_launch pick every 4-bit instantiation of both kernels: the dot form <1, 2, 4, 8, 16> and all 14
    <MB, NR, DEEP> forms of the matrix-core kernel (PLAIN names the form each shape runs); the torch op on one of them."""
    x, p, s, wh = _rand_problem(M, N, K, seed=M * 131 + N + K)
    ref, absdot = _dots(x, wh)
    tol = C.linear_tol(ref, absdot, K)
    y4 = hip.linear_w4(x, p, s)
    y16 = hip.linear(x, wh)
    torch.cuda.synchronize()
    _check(y4, ref, tol, f"w4 {what}")
    _check(y16, ref, tol, f"bf16 on W^, {M}x{N}x{K}")
    if (M, N, K) == (5, 64, 4096):
        import thinkdiff.ops  # noqa: F401
        assert torch.equal(torch.ops.thinkdiff_hip.linear_w4(x, p, s, None, 0, None, None), y4)


# ---- 5. epilogues ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(4, 64, 1536), (33, 64, 2048)])
def test_linear_w4_bias_act_residual(hip, M, N, K):
    """y = bf16(bf16(silu(bf16(acc + bias))) + res): the Linear output rounds, the activation rounds, the residual sum rounds.  silu has slope <= 1.1
    and is evaluated in fp32 with v_exp / v_rcp (<= 2^-20 relative, generous).  M = 4: MFMA <1, 1>; M = 33: MFMA <3, 1>.  Without the activation the
    8-bit tests' bound: one ulp each for the inner value and the sum."""
    x, p, s, wh = _rand_problem(M, N, K, seed=M + K)
    g = torch.Generator().manual_seed(7)
    bias = torch.randn(N, generator=g).bfloat16().cuda()
    res = torch.randn(M, N, generator=g).bfloat16().cuda()
    dot, absdot = _dots(x, wh)
    inner = dot + bias.double()
    ref = _r16(inner) + res.double()
    tol = C.ulp_bf16(ref) + C.ulp_bf16(inner) + C.sum_bound(K, absdot)
    y4 = hip.linear_w4(x, p, s, bias=bias, res=res)
    y16 = hip.linear(x, wh, bias=bias, res=res)
    torch.cuda.synchronize()
    _check(y4, ref, tol, "w4 bias + residual")
    _check(y16, ref, tol, "bf16 bias + residual")
    # the residual may be the output itself (the engine's h += ...)
    out = res.clone()
    hip.linear_w4(x, p, s, bias=bias, res=out, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, y4)
    # ... with SiLU between the Linear and the residual
    i16 = _r16(inner)
    a_ref = i16 * torch.sigmoid(i16)
    ref = _r16(a_ref) + res.double()
    d_in = C.sum_bound(K, absdot) + C.ulp_bf16(inner)
    d_act = 1.1 * d_in + 2.0 ** -20 * a_ref.abs() + C.ulp_bf16(a_ref)
    tol = C.ulp_bf16(ref) + d_act
    y4 = hip.linear_w4(x, p, s, bias=bias, act=hip.ACT_SILU, res=res)
    y16 = hip.linear(x, wh, bias=bias, act=hip.ACT_SILU, res=res)
    torch.cuda.synchronize()
    _check(y4, ref, tol, "w4 bias + silu + residual")
    _check(y16, ref, tol, "bf16 bias + silu + residual")


@pytest.mark.parametrize("M,N,K,n_split", [(1, 96, 1536, 64), (48, 96, 1024, 64)])
def test_linear_w4_split_output(hip, M, N, K, n_split):
    """Columns < n_split to one buffer, the rest to another (the q | k|v projection's form), with bias: no further rounding point."""
    x, p, s, wh = _rand_problem(M, N, K, seed=M + N)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(5)).bfloat16().cuda()
    dot, absdot = _dots(x, wh)
    ref = dot + bias.double()
    tol = C.linear_tol(ref, absdot, K)
    for fn, args, what in ((hip.linear_split_w4, (x, p, s), "w4"), (hip.linear_split, (x, wh), "bf16")):
        y0 = torch.zeros(M, n_split, dtype=torch.bfloat16, device="cuda")
        y1 = torch.zeros(M, N - n_split, dtype=torch.bfloat16, device="cuda")
        fn(*args, bias, y0, 0, y1, 0, n_split)
        torch.cuda.synchronize()
        _check(torch.cat([y0, y1], dim=1), ref, tol, f"{what} split output")


@pytest.mark.parametrize("M,inter,K", [(2, 64, 1536), (8, 40, 96), (17, 64, 1024), (33, 2048, 4096), (5, 64, 2048)])
def test_linear_w4_glu(hip, M, inter, K):
    """out = bf16(bf16(silu(bf16(g))) * bf16(u)), g / u = x . gate / up rows.  M = 2, 8 (K = 96): dot form; then the matrix-core kernel gated (blocks = inter / 8):
    17 x 64: <2, 1, shallow>; 33 x 2048 x 4096: <3, 1, shallow> (16 steps); 5 x 64 x 2048: <1, 1, shallow>.  The gated mode changes which weight rows and scale
    bytes a block addresses and the epilogue, none of which depends on MB or DEEP; the loop forms themselves are all run plain above.
    Bound, carried through the chain (the 8-bit tests' composition): dg = sum bound + ulp(g); ds = 1.1 dg + 2^-20 |s| + ulp(s); du = sum bound + ulp(u);
    product: |s| du + |u| ds + ds du; plus the output's ulp."""
    x, p, s, wh = _rand_problem(M, 2 * inter, K, seed=M + inter)
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
    y4 = hip.linear_glu_w4(x, p, s)
    y16 = hip.linear_glu(x, wh)
    torch.cuda.synchronize()
    _check(y4, ref, tol, "w4 gated")
    _check(y16, ref, tol, "bf16 gated")


# ---- 6. the engine ---------------------------------------------------------------------------------------------------------------------------
LINEAR_KEYS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "gate_proj.weight", "up_proj.weight", "down_proj.weight")


def _is_quantised(k, cfg):
    return k.endswith(LINEAR_KEYS) or k == "lm_head.weight" or (cfg.tie_embeddings and k == "model.embed_tokens.weight")


def _hat_state_dict(sd, cfg):
    """The oracle's weights of the quantised model: W^ from the restatement for every Linear the engine quantises (the blocks run along K: quantising
    q / k / v or gate / up separately equals quantising the fused matrices), lm_head -- and with tied embeddings the embedding table, which is it."""
    return {k: (C.quantize_blocks(v)[2].to(v.dtype) if _is_quantised(k, cfg) else v) for k, v in sd.items()}


def _engine(cfg, sd, max_len, quantization=None):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    e = Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                                            num_key_value_heads=cfg.num_kv_heads, intermediate_size=cfg.intermediate, vocab_size=cfg.vocab,
                                            tie_word_embeddings=cfg.tie_embeddings), max_model_len=max_len)
    e.weight_quantization = quantization
    e.load_state_dict(sd)
    return e


@pytest.mark.parametrize("tie", [False, True])
def test_engine_decode_with_mxfp4_weights(hip, tie):
    cfg = Q.tiny_config(tie_embeddings=tie)
    sd = Q.init_weights(cfg, seed=31 + int(tie))
    sd_hat = _hat_state_dict(sd, cfg)
    n0, BMAX, SLOTS = 40, 64, 66
    e = _engine(cfg, sd, max_len=SLOTS * 128)
    assert e.weight_info() == {"mode": "bf16", "stream_on": False, "bytes_8bit": 0, "n_linears": 0}
    with pytest.raises(hip.ThinkDiffHipError, match="not quantised"):
        e.set_weight_stream(True)
    e.quantize_weights("mxfp4")
    D, I, NQKV = cfg.hidden, cfg.intermediate, (cfg.num_heads + 2 * cfg.num_kv_heads) * 128
    elems = cfg.num_layers * (NQKV * D + D * cfg.num_heads * 128 + 2 * I * D + D * I) + cfg.vocab * D
    assert e.weight_info() == {"mode": "mxfp4", "stream_on": True, "bytes_8bit": elems // 2 + elems // 32, "n_linears": 4 * cfg.num_layers + 1}
    e.set_slots(SLOTS)
    assert e.slot_len == 128
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
    assert _rel(hid_p, p16) < 2e-2                                   # the prefill (bf16 W^ on the tiles, 4-bit stream for its 40-row Linears)
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

    # The outputs cannot tell the 4-bit kernels from the bf16 kernels on W^ (same model, often the same bits), so the handle counts the launches that
    # read the copy: step() is 3 calls = an eager step and a captured one (2 x (4 Linears per layer + lm_head)) and a replay, which counts nothing
    per_step = 4 * cfg.num_layers + 1
    for B in (1, 3, 17, 64):
        assert e.set_weight_stream(True) in (True, False)
        n_before = e.weight_stream_launches()
        on_h, on_l = step(B)
        n_on = e.weight_stream_launches() - n_before
        assert n_on in (2 * per_step, 3 * per_step), f"the decode step read the 4-bit copy in {n_on} launches"     # (3 x: a runtime that cannot capture)
        assert e.set_weight_stream(False) is True
        off_h, off_l = step(B)
        assert e.weight_stream_launches() - n_before == n_on, "stream off still read the 4-bit copy"
        e.set_weight_stream(True)
        eref = _rel(ref16[:B], ref32[:B])
        for name, h, lg in (("stream on", on_h, on_l), ("stream off", off_h, off_l)):
            e16, e32 = _rel(h, ref16[:B]), _rel(h, ref32[:B])
            print(f"B={B} {name}: rel-RMSE hip~bf16 {e16:.4f} hip~fp32 {e32:.4f} bf16~fp32 {eref:.4f}")
            assert e16 < 2e-2 and e32 < 1.5 * eref + 2e-3
            assert _rel(lg, lref[:B]) < 3e-2
        # ... and the same assertions with the stream-off result in the bf16 oracle's place
        assert _rel(on_h, off_h) < 2e-2 and _rel(on_h, ref32[:B]) < 1.5 * _rel(off_h, ref32[:B]) + 2e-3
        assert _rel(on_l, off_l) < 3e-2

    # more than 64 rows never read the 4-bit copy: identical bits with the stream on and off
    n1 = 100
    p1 = torch.randint(0, cfg.vocab, (n1,), generator=g).to(torch.int32)
    wide = {}
    n_before = e.weight_stream_launches()
    for on in (True, False):
        e.set_weight_stream(on)
        wide[on] = (step(65), (e.forward(Q.text_position_ids(n1), p1, slot=65)[0].clone(),))
        torch.cuda.synchronize()
    for a, b in zip(wide[True][0] + wide[True][1], wide[False][0] + wide[False][1]):
        assert torch.equal(a, b)
    assert e.weight_stream_launches() == n_before          # ... and none of these launches read it
    e.set_weight_stream(True)

    # quantising twice leaves the decode output bit-equal
    before = step(17)
    e.quantize_weights("mxfp4")
    assert e.weight_info()["stream_on"] is True
    after = step(17)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])

    # the other format is refused, naming both: the arena holds W^ of this one, not the weights that were loaded
    with pytest.raises(hip.ThinkDiffHipError, match="TD_QWEN2_WEIGHTS_MXFP4.*TD_QWEN2_WEIGHTS_E4M3"):
        e.quantize_weights("fp8")
    assert e.weight_info()["mode"] == "mxfp4"
    again = step(17)
    assert torch.equal(before[0], again[0]) and torch.equal(before[1], again[1])

    # parameters loaded behind the quantiser's back: every run is refused, by name, until the weights are quantised again
    e.load_state_dict(sd)
    for call in (lambda: e.decode_batch(toks[:3], torch.full((3, 3), n0, dtype=torch.int32), [n0] * 3),
                 lambda: e.forward(pos, prompt, slot=0)):
        with pytest.raises(hip.ThinkDiffHipError, match="td_qwen2_quantize_weights"):
            call()
    e.quantize_weights("mxfp4")
    again = step(17)
    assert torch.equal(before[0], again[0]) and torch.equal(before[1], again[1])


def test_fp8_handle_refuses_mxfp4_until_reloaded(hip):
    cfg = Q.tiny_config()
    sd = Q.init_weights(cfg, seed=5)
    e = _engine(cfg, sd, max_len=128)
    e.quantize_weights("fp8")
    with pytest.raises(hip.ThinkDiffHipError, match="TD_QWEN2_WEIGHTS_E4M3.*TD_QWEN2_WEIGHTS_MXFP4"):
        e.quantize_weights("mxfp4")
    assert e.weight_info()["mode"] == "fp8"
    # with its parameters loaded again the handle takes the other format, and is then the handle a fresh engine would be
    e.load_state_dict(sd)
    e.quantize_weights("mxfp4")
    fresh = _engine(cfg, sd, max_len=128, quantization="mxfp4")
    assert e.weight_info() == fresh.weight_info() and e.weight_info()["mode"] == "mxfp4"
    prompt = torch.arange(7, 27, dtype=torch.int32)
    a, b = e.forward(Q.text_position_ids(20), prompt, slot=0)[0], fresh.forward(Q.text_position_ids(20), prompt, slot=0)[0]
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ---- 7. pre-quantised checkpoints ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", [False, True])
def test_prequantised_state_dict_loads_exactly(hip, tie):
    """The tiny state dict quantised by the restatement, once under the OCP rule and once with every exponent one higher, loaded as
    `weight` uint8 [N, K / 2] + `weight_scale` uint8 [N, K / 32]: prefill and decode outputs equal, bit for bit, the run from the dequantised bf16
    state dict (the engine has no parameter read-back entry; the outputs see every Linear)."""
    cfg = Q.tiny_config(tie_embeddings=tie)
    sd = Q.init_weights(cfg, seed=77 + int(tie))
    prompt = torch.randint(0, cfg.vocab, (24,), generator=torch.Generator().manual_seed(1)).to(torch.int32)

    def run(state):
        e = _engine(cfg, state, max_len=128, quantization="mxfp4")
        assert e.weight_info()["mode"] == "mxfp4" and e.weight_info()["stream_on"]
        h, _ = e.forward(Q.text_position_ids(24), prompt, slot=0)
        d = e.decode_batch(torch.tensor([5], dtype=torch.int32), torch.full((3, 1), 24, dtype=torch.int32), [24])
        torch.cuda.synchronize()
        return h.clone(), d[0].clone(), d[1].clone()

    for bump in (0, 1):
        packed_sd, hat_sd = {}, {}
        for k, v in sd.items():
            if k.endswith(LINEAR_KEYS) or k == "lm_head.weight":
                p, s, wh, _ = C.quantize_blocks(v, bump=bump)
                packed_sd[k], packed_sd[k + "_scale"], hat_sd[k] = p, s, wh.to(v.dtype)
            else:
                packed_sd[k] = hat_sd[k] = v
        got, want = run(packed_sd), run(hat_sd)
        for a, b in zip(got, want):
            assert torch.equal(a, b), f"bump={bump}: the packed load is not the run from the dequantised weights"
    # on an engine that is not in this mode a packed tensor is refused by name
    with pytest.raises(ValueError, match=r"weight' is a packed MXFP4 tensor.*'fp8'"):
        _engine(cfg, packed_sd, max_len=128, quantization="fp8")


# ---- 8. get_embed ----------------------------------------------------------------------------------------------------------------------------
def test_get_embed_with_mxfp4_quantization(hip):
    """ThinkDiff-LVLM get_embed, teacher-forced as tests/test_qwen2_gpu.py::test_get_embed_teacher_forced, with vllm_config["quantization"] = "mxfp4":
    the aligner restatement on the oracle run on W^, within that test's 3e-2."""
    from oracle import aligner_ref as A
    from thinkdiff.models.mllama_vllm_t5_embed_decoder_2 import MllamaVllmT5EmbedDecoderForConditionalGeneration_5
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig
    cfg = Q.tiny_config()
    sd = Q.init_weights(cfg, seed=9)
    sd_hat = _hat_state_dict(sd, cfg)
    asd = A.init_weights(cfg.hidden, 4096, seed=4)
    tc = Qwen2VLTextConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                           num_key_value_heads=cfg.num_kv_heads, intermediate_size=cfg.intermediate, vocab_size=cfg.vocab)
    base = {"max_model_len": 256, "max_tokens": 6, "min_tokens": 6}
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, cfg.vocab, (20,), generator=g).tolist()
    forced = torch.randint(0, cfg.vocab, (6,), generator=g).tolist()

    def run(m, et="both"):
        embs, texts = m.get_embed([{"prompt_token_ids": prompt}], embedding_type=et, need_process=False, forced_output_ids=[forced])
        torch.cuda.synchronize()
        assert texts == [" ".join(map(str, forced))]
        return embs[0].clone()

    def ref_aligner(h):
        F = torch.nn.functional
        y = F.linear(F.gelu(F.linear(h, asd["mm_projector.0.weight"], asd["mm_projector.0.bias"])), asd["mm_projector.2.weight"], asd["mm_projector.2.bias"])
        return A.t5_layer_norm(y.float(), asd["mm_projector.3.weight"].float()).bfloat16()

    m4 = MllamaVllmT5EmbedDecoderForConditionalGeneration_5(tc, vllm_config={**base, "quantization": "mxfp4"})
    m4.mllama.load_state_dict(sd)          # (with the key set this ends with the quantisation: the handle is never left stale)
    m4.load_state_dict(asd)
    assert m4.mllama.weight_info()["mode"] == "mxfp4" and m4.mllama.weight_info()["stream_on"]
    ref_h, _ = Q.text_model_hidden(sd_hat, cfg, Q.text_position_ids(26), token_ids=torch.tensor(prompt + forced))
    for et, sl in [("both", slice(0, 26)), ("output_embed", slice(20, 26))]:
        got = run(m4, et)
        assert got.shape == (sl.stop - sl.start, 4096)
        assert _rel(got, ref_aligner(ref_h[sl])) < 3e-2
    # a later load re-quantises instead of leaving the handle stale
    m4.mllama.load_state_dict(sd)
    assert _rel(run(m4), ref_aligner(ref_h)) < 3e-2
