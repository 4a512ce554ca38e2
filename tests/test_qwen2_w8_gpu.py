"""The 8-bit weight stream of the Qwen2-VL decode engine on the GPU: the quantiser bit for bit against the CPU restatement
(tests/qwen2_w8_common.py), the 8-bit forms of both weight-stream kernels (csrc/gemv_bf16.hip) exactly on integer operands and against float64
on random ones, and the engine / get_embed with quantised weights against the oracle run on the dequantised weights W^.

Random-operand bound (linear_tol): the kernels form exact products (bf16 x W^, both bf16 values) and add them in fp32 in some order, then round
once: |y - ref| <= ulp_bf16(ref) + K 2^-24 sum_k |x_k w^_k|.  Every further rounding point of an epilogue adds its own ulp, carried to the output
(the composition tests/test_epilogues_gpu.py uses).  The SAME bound is applied to the bf16 kernels on W^ at the same shape: a wrong bound fails there too.
"""
import pytest
import torch

import qwen2_w8_common as C
from oracle import qwen2vl_ref as Q

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


# ---- 1. the quantiser ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 19, 64])
@pytest.mark.parametrize("K", [128, 1536, 8960])
def test_quantiser_is_bit_exact(hip, N, K):
    w = C.edge_rows(N, K, seed=3 * N + K)
    q_ref, s_ref, wh_ref, _ = C.quantize_rows(w)
    wd = w.cuda()
    q, s, wh = hip.quant_weight_rows_e4m3(wd)
    torch.cuda.synchronize()
    assert torch.equal(s.cpu(), s_ref)
    assert torch.equal(q.cpu(), q_ref)
    assert torch.equal(wh.cpu().float(), wh_ref)
    assert torch.equal(wd.cpu(), w)                                   # the input is untouched unless aliased
    # no W^ wanted; W^ over the input (a strided view: the row stride is not K)
    q2, s2, none = hip.quant_weight_rows_e4m3(wd, want_w_hat=False)
    assert none is None and torch.equal(q2, q) and torch.equal(s2, s)
    wide = torch.full((N, K + 64), 7.0, dtype=torch.bfloat16, device="cuda")
    wide[:, :K] = wd
    q3, s3, wh3 = hip.quant_weight_rows_e4m3(wide[:, :K], inplace=True)
    torch.cuda.synchronize()
    assert wh3.data_ptr() == wide.data_ptr() and torch.equal(q3, q) and torch.equal(s3, s)
    assert torch.equal(wide[:, :K].cpu().float(), wh_ref) and bool((wide[:, K:] == 7.0).all())
    # quantising W^ gives W^
    q4, s4, wh4 = hip.quant_weight_rows_e4m3(wh)
    assert torch.equal(wh4, wh)
    # the torch op says the same
    import thinkdiff.ops  # noqa: F401
    qo, so, who = torch.ops.thinkdiff_hip.quant_weight_rows_e4m3(wd)
    assert torch.equal(qo, q) and torch.equal(so, s) and torch.equal(who, wh)


def test_quantiser_saturates_a_row_beyond_the_exponent_clamp(hip):
    """amax > 448 x 2^40 (no real weight): e_n is clamped at 40 and the scaled values beyond 448 saturate to +-448 (byte 0x7E / 0xFE) instead of
    reaching the conversion out of range; values of that row inside the range quantise as usual, other rows are untouched."""
    w = torch.zeros(2, 128)
    w[0, 0], w[0, 1], w[0, 2], w[0, 3] = 2.0 ** 60, -(2.0 ** 55), 3.0 * 2.0 ** 40, -(2.0 ** 31)
    w[1] = torch.linspace(-1, 1, 128)
    q, s, wh = hip.quant_weight_rows_e4m3(w.bfloat16().cuda())
    torch.cuda.synchronize()
    assert float(s[0]) == 2.0 ** 40 and q[0, :4].tolist() == [0x7E, 0xFE, 0x44, 0x80 | 0x01]      # 448, -448, 3 = 1.5 x 2^1, -2^-9
    assert wh[0, :4].float().tolist() == [448.0 * 2.0 ** 40, -448.0 * 2.0 ** 40, 3.0 * 2.0 ** 40, -(2.0 ** 31)]
    q_ref, s_ref, wh_ref, _ = C.quantize_rows(w.bfloat16()[1:])
    assert torch.equal(q[1:].cpu(), q_ref) and torch.equal(s[1:].cpu(), s_ref) and torch.equal(wh[1:].cpu().float(), wh_ref)


# ---- 2. exact integers -----------------------------------------------------------------------------------------------------------------------
def _int_problem(N, K):
    """W[n, k] = small integer x 2^e_n with e_n from -6 to 6, depending on n and k differently; every value is an e4m3 value times a power of two,
    so the restatement reproduces W exactly and every fp32 sum of x W products is exact (|sum| 2^-e_n < 2^24)."""
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    wi = ((3 * n + 5 * k + (n * k) % 7) % 15 - 7).float()
    e = (torch.arange(N) % 13 - 6)
    w = wi * torch.exp2(e.float())[:, None]
    q, s, wh, _ = C.quantize_rows(w)
    assert torch.equal(wh, w)
    return w, q.cuda(), s.cuda()


@pytest.mark.parametrize("N,K", [(64, 8960), (48, 384)])
def test_linear_w8_exact_integers(hip, N, K):
    w, q, s = _int_problem(N, K)
    for M in (1, 3, 4, 5, 16, 17, 33, 64):
        m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
        x = ((2 * m + 3 * k + (m * k) % 5) % 9 - 4).float()
        ref = (x.double() @ w.double().T).float().bfloat16()           # bf16(float64 result): the float64 sum is exact too
        y = hip.linear_w8(x.bfloat16().cuda(), q, s)
        torch.cuda.synchronize()
        assert torch.equal(y.cpu(), ref), f"M={M}: {int((y.cpu() != ref).sum())} elements differ"
        # one-hot rows read single weights back: y[m, n] = W[n, k_m]
        km = (37 * torch.arange(M) + 11) % K
        x1 = torch.zeros(M, K)
        x1[torch.arange(M), km] = 1.0
        y1 = hip.linear_w8(x1.bfloat16().cuda(), q, s)
        torch.cuda.synchronize()
        assert torch.equal(y1.cpu().float(), w[:, km].T.contiguous()), f"M={M}: one-hot rows do not read W[n, k_m] back"


# ---- 3. random operands vs float64 on (x, W^) ----------------------------------------------------------------------------------------------
_WEIGHTS = {}


def _rand_weight(N, K):
    """Random weights with row magnitudes spread over 2^-3 .. 2^3, quantised by the restatement; made once per (N, K) and shared, unchanged, by the
    cases of that extent (the last one stays on the device: the large extents take a second to make on the host)."""
    if (N, K) not in _WEIGHTS:
        _WEIGHTS.clear()
        g = torch.Generator().manual_seed(1000003 * N + K)
        w = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-3, 4, (N, 1), generator=g).float()) * 0.05).bfloat16()
        q, s, wh, _ = C.quantize_rows(w)
        _WEIGHTS[(N, K)] = (q.cuda(), s.cuda(), wh.bfloat16().cuda())
    return _WEIGHTS[(N, K)]


def _rand_problem(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).bfloat16()
    q, s, wh = _rand_weight(N, K)
    return x.cuda(), q, s, wh


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
    (4, 64, 8960, "dot form <4>: main loop and tail"),
    (3, 64, 128, "dot form <4>: K too short for the main loop"),
    (8, 40, 192, "dot form <8>: 5 .. 8 rows of a shape the matrix core does not take (K % 128, N % 16)"),
    (13, 40, 192, "dot form <16>"),
    # the matrix-core form <MB, NR, DEEP>: MB = ceil(M / 16); NR = 2 from 1024 weight blocks (N >= 16384) on, for MB > 1; DEEP when a workgroup
    # has at least 32 of the 128-element steps (K / 128 / ks, ks = K parts = min(8, 512 / blocks, steps / 8) below 256 blocks): all 14 forms
    (5, 64, 2048, "MFMA <1, 1, shallow> with K split over 2 workgroups"),
    (16, 4096, 4096, "MFMA <1, 1, DEEP>"),
    (17, 64, 2048, "MFMA <2, 1, shallow>, K split"),
    (17, 4096, 4096, "MFMA <2, 1, DEEP>"),
    (48, 256, 1024, "MFMA <3, 1, shallow>"),
    (48, 3584, 8192, "MFMA <3, 1, DEEP> with K split over 2 workgroups (the 7B down_proj's form: 224 blocks)"),
    (64, 320, 512, "MFMA <4, 1, shallow>"),
    (64, 64, 8960, "MFMA <4, 1, shallow> with K split over 8 workgroups"),
    (64, 3584, 8192, "MFMA <4, 1, DEEP> with K split over 2 workgroups"),
    (17, 16384, 128, "MFMA <2, 2, shallow>: two weight blocks per workgroup"),
    (48, 16384, 128, "MFMA <3, 2, shallow> (lm_head's form at 33 - 48 sequences)"),
    (64, 16384, 128, "MFMA <4, 2, shallow>"),
    (17, 16384, 4096, "MFMA <2, 2, DEEP>"),
    (33, 16384, 4096, "MFMA <3, 2, DEEP>"),
    (64, 16384, 4096, "MFMA <4, 2, DEEP>"),
]


@pytest.mark.parametrize("M,N,K,what", PLAIN, ids=[f"{m}x{n}x{k}" for m, n, k, _ in PLAIN])
def test_linear_w8_random_vs_float64(hip, M, N, K, what):
    """Plain Linear at shapes that make td_gemv_launch pick every instantiation of both kernels: the dot form <1, 2, 4, 8, 16> and all 14
    <MB, NR, DEEP> forms of the matrix-core kernel (PLAIN names the form each shape runs); the torch op on one of them."""
    x, q, s, wh = _rand_problem(M, N, K, seed=M * 131 + N + K)
    ref, absdot = _dots(x, wh)
    tol = C.linear_tol(ref, absdot, K)
    y8 = hip.linear_w8(x, q, s)
    y16 = hip.linear(x, wh)
    torch.cuda.synchronize()
    _check(y8, ref, tol, f"w8 {what}")
    _check(y16, ref, tol, f"bf16 on W^, {M}x{N}x{K}")
    if (M, N, K) == (5, 64, 2048):
        import thinkdiff.ops  # noqa: F401
        assert torch.equal(torch.ops.thinkdiff_hip.linear_w8(x, q, s, None, 0, None, None), y8)


@pytest.mark.parametrize("M,N,K", [(4, 64, 1536), (33, 64, 2048)])
def test_linear_w8_bias_residual(hip, M, N, K):
    """y = bf16(bf16(acc + bias) + res): the Linear output rounds, then the residual sum rounds -- one ulp each, the first at the inner value.
    M = 4: dot form; M = 33: MFMA <3, 1> with K split (the ticket hand-off's finisher runs the epilogue)."""
    x, q, s, wh = _rand_problem(M, N, K, seed=M + K)
    g = torch.Generator().manual_seed(7)
    bias = torch.randn(N, generator=g).bfloat16().cuda()
    res = torch.randn(M, N, generator=g).bfloat16().cuda()
    dot, absdot = _dots(x, wh)
    inner = dot + bias.double()
    ref = _r16(inner) + res.double()
    tol = C.ulp_bf16(ref) + C.ulp_bf16(inner) + C.sum_bound(K, absdot)
    y8 = hip.linear_w8(x, q, s, bias=bias, res=res)
    y16 = hip.linear(x, wh, bias=bias, res=res)
    torch.cuda.synchronize()
    _check(y8, ref, tol, "w8 bias + residual")
    _check(y16, ref, tol, "bf16 bias + residual")
    # the residual may be the output itself (the engine's h += ...)
    out = res.clone()
    hip.linear_w8(x, q, s, bias=bias, res=out, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, y8)


@pytest.mark.parametrize("M,N,K,n_split", [(1, 96, 1536, 64), (48, 96, 1024, 64)])
def test_linear_w8_split_output(hip, M, N, K, n_split):
    """Columns < n_split to one buffer, the rest to another (the q | k|v projection's form), with bias: no further rounding point."""
    x, q, s, wh = _rand_problem(M, N, K, seed=M + N)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(5)).bfloat16().cuda()
    dot, absdot = _dots(x, wh)
    ref = dot + bias.double()
    tol = C.linear_tol(ref, absdot, K)
    for fn, args, what in ((hip.linear_split_w8, (x, q, s), "w8"), (hip.linear_split, (x, wh), "bf16")):
        y0 = torch.zeros(M, n_split, dtype=torch.bfloat16, device="cuda")
        y1 = torch.zeros(M, N - n_split, dtype=torch.bfloat16, device="cuda")
        fn(*args, bias, y0, 0, y1, 0, n_split)
        torch.cuda.synchronize()
        _check(torch.cat([y0, y1], dim=1), ref, tol, f"{what} split output")


@pytest.mark.parametrize("M,inter,K", [(2, 64, 1536), (8, 40, 48), (17, 64, 1024), (64, 8192, 512), (33, 2048, 4096), (64, 8192, 4096), (5, 64, 2048)])
def test_linear_w8_glu(hip, M, inter, K):
    """out = bf16(bf16(silu(bf16(g))) * bf16(u)), g / u = x . gate / up rows.  M = 2, 8: dot form; then the matrix-core kernel gated (blocks = inter / 8):
    17 x 64: <2, 1, shallow>; 64 x 8192 x 512: <4, 2, shallow>; 33 x 2048 x 4096: <3, 1, DEEP>; 64 x 8192 x 4096: <4, 2, DEEP>; 5 x 64 x 2048: <1, 1, shallow>
    with K split over 2 workgroups (one activation block, and the ticket hand-off's finisher running the gated epilogue).  Not every
    <MB, NR, DEEP> is run gated: the gated mode changes which weight rows and scales a block addresses and the epilogue, none of which depends on
    MB or DEEP beyond what these five cover (both NR, both depths, one, an odd and a full MB); the loop forms themselves are all run plain above.
    Bound, carried through the chain: dg = sum bound + ulp(g); silu has slope <= 1.1 and is evaluated in fp32 with v_exp / v_rcp (<= 2^-20 relative,
    generous): ds = 1.1 dg + 2^-20 |s| + ulp(s); du = sum bound + ulp(u); product: |s| du + |u| ds + ds du; plus the output's ulp."""
    x, q, s, wh = _rand_problem(M, 2 * inter, K, seed=M + inter)
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
    y8 = hip.linear_glu_w8(x, q, s)
    y16 = hip.linear_glu(x, wh)
    torch.cuda.synchronize()
    _check(y8, ref, tol, "w8 gated")
    _check(y16, ref, tol, "bf16 gated")


# ---- 4. the engine ---------------------------------------------------------------------------------------------------------------------------
LINEAR_KEYS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "gate_proj.weight", "up_proj.weight", "down_proj.weight")


def _hat_state_dict(sd, cfg):
    """The oracle's weights of the quantised model: W^ from the restatement for every Linear the engine quantises (per-row scales: quantising
    q / k / v or gate / up separately equals quantising the fused matrices), lm_head -- and with tied embeddings the embedding table, which is it."""
    out = {}
    for k, v in sd.items():
        quant = k.endswith(LINEAR_KEYS) or k == "lm_head.weight" or (cfg.tie_embeddings and k == "model.embed_tokens.weight")
        out[k] = C.quantize_rows(v)[2].to(v.dtype) if quant else v
    return out


def _engine(cfg, sd, max_len):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    e = Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                                            num_key_value_heads=cfg.num_kv_heads, intermediate_size=cfg.intermediate, vocab_size=cfg.vocab,
                                            tie_word_embeddings=cfg.tie_embeddings), max_model_len=max_len)
    e.load_state_dict(sd)
    return e


@pytest.mark.parametrize("tie", [False, True])
def test_engine_decode_with_quantised_weights(hip, tie):
    cfg = Q.tiny_config(tie_embeddings=tie)
    sd = Q.init_weights(cfg, seed=31 + int(tie))
    sd_hat = _hat_state_dict(sd, cfg)
    n0, BMAX, SLOTS = 40, 64, 66
    e = _engine(cfg, sd, max_len=SLOTS * 128)
    assert e.weight_info() == {"mode": "bf16", "stream_on": False, "bytes_8bit": 0, "n_linears": 0}
    with pytest.raises(hip.ThinkDiffHipError, match="not quantised"):
        e.set_weight_stream(True)
    e.quantize_weights("fp8")
    D, I, NQKV = cfg.hidden, cfg.intermediate, (cfg.num_heads + 2 * cfg.num_kv_heads) * 128
    elems = cfg.num_layers * (NQKV * D + D * cfg.num_heads * 128 + 2 * I * D + D * I) + cfg.vocab * D
    rows = cfg.num_layers * (NQKV + D + 2 * I + D) + cfg.vocab
    assert e.weight_info() == {"mode": "fp8", "stream_on": True, "bytes_8bit": elems + 4 * rows, "n_linears": 4 * cfg.num_layers + 1}
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
    assert _rel(hid_p, p16) < 2e-2                                   # the prefill (bf16 W^ on the tiles, 8-bit stream for its 40-row Linears)
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

    # The outputs cannot tell the 8-bit kernels from the bf16 kernels on W^ (same model, often the same bits), so the handle counts the launches that
    # read the 8-bit copy: step() is 3 calls = an eager step and a captured one (2 x (4 Linears per layer + lm_head)) and a replay, which counts nothing
    per_step = 4 * cfg.num_layers + 1
    for B in (1, 3, 17, 64):
        assert e.set_weight_stream(True) in (True, False)
        n_before = e.weight_stream_launches()
        on_h, on_l = step(B)
        n_on = e.weight_stream_launches() - n_before
        assert n_on in (2 * per_step, 3 * per_step), f"the decode step read the 8-bit copy in {n_on} launches"     # (3 x: a runtime that cannot capture)
        assert e.set_weight_stream(False) is True
        off_h, off_l = step(B)
        assert e.weight_stream_launches() - n_before == n_on, "stream off still read the 8-bit copy"
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

    # more than 64 rows never read the 8-bit copy: identical bits with the stream on and off
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
    e.quantize_weights("fp8")
    assert e.weight_info()["stream_on"] is True
    after = step(17)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])

    # parameters loaded behind the quantiser's back: every run is refused, by name, until the weights are quantised again
    e.load_state_dict(sd)
    for call in (lambda: e.decode_batch(toks[:3], torch.full((3, 3), n0, dtype=torch.int32), [n0] * 3),
                 lambda: e.forward(pos, prompt, slot=0)):
        with pytest.raises(hip.ThinkDiffHipError, match="td_qwen2_quantize_weights"):
            call()
    e.quantize_weights("fp8")
    again = step(17)
    assert torch.equal(before[0], again[0]) and torch.equal(before[1], again[1])


# ---- 5. get_embed ----------------------------------------------------------------------------------------------------------------------------
def test_get_embed_with_fp8_quantization(hip):
    """ThinkDiff-LVLM get_embed, teacher-forced as tests/test_qwen2_gpu.py::test_get_embed_teacher_forced, with vllm_config["quantization"] = "fp8":
    the aligner restatement on the oracle run on W^, within that test's 3e-2; without the key the model is bit-equal to one built as before."""
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

    def build(vc):
        m = MllamaVllmT5EmbedDecoderForConditionalGeneration_5(tc, vllm_config=vc)
        m.mllama.load_state_dict(sd)          # (with the key set this ends with the quantisation: the handle is never left stale)
        m.load_state_dict(asd)
        return m

    def run(m, et="both"):
        embs, texts = m.get_embed([{"prompt_token_ids": prompt}], embedding_type=et, need_process=False, forced_output_ids=[forced])
        torch.cuda.synchronize()
        assert texts == [" ".join(map(str, forced))]
        return embs[0].clone()

    def ref_aligner(h):
        F = torch.nn.functional
        y = F.linear(F.gelu(F.linear(h, asd["mm_projector.0.weight"], asd["mm_projector.0.bias"])), asd["mm_projector.2.weight"], asd["mm_projector.2.bias"])
        return A.t5_layer_norm(y.float(), asd["mm_projector.3.weight"].float()).bfloat16()

    m8 = build({**base, "quantization": "fp8"})
    assert m8.mllama.weight_info()["mode"] == "fp8" and m8.mllama.weight_info()["stream_on"]
    ref_h, _ = Q.text_model_hidden(sd_hat, cfg, Q.text_position_ids(26), token_ids=torch.tensor(prompt + forced))
    for et, sl in [("both", slice(0, 26)), ("output_embed", slice(20, 26))]:
        got = run(m8, et)
        assert got.shape == (sl.stop - sl.start, 4096)
        assert _rel(got, ref_aligner(ref_h[sl])) < 3e-2
    # a later load re-quantises instead of leaving the handle stale
    m8.mllama.load_state_dict(sd)
    assert _rel(run(m8), ref_aligner(ref_h)) < 3e-2
    del m8
    # no key, or None: today's model, bit for bit
    a, b = run(build(dict(base))), run(build({**base, "quantization": None}))
    assert torch.equal(a, b)
    plain = MllamaVllmT5EmbedDecoderForConditionalGeneration_5(tc, vllm_config=dict(base))
    assert plain.mllama.weight_quantization is None and plain.mllama.weight_info()["mode"] == "bf16"
