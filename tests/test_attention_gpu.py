"""GPU parity of the fused attention kernel (td_attention_bf16) vs fp32 torch CPU softmax(QK^T)V.

Tolerance: P is rounded to bf16 before the PV product (as in flash-style kernels the reference's
SDPA dispatches to) and the output is bf16: |err| <= 2^-7 of the output scale.

The score-bias tests (td_attention_bias_bf16, at the end) keep that bar against a float64 softmax(q.k^T scale + bias [+ causal mask]) . v:
the bias joins the fp32 scores before the softmax (as bias / scale in the kernel's unscaled domain, fp32: ~2^-24 relative, nothing
next to the bf16 rounding of P), so the error model is the one above.  What makes them decisive is the INPUT: a bias that is independent
per (head, row, key) and as large as the q.k scores, checked on the CPU to move the reference by >= 10x the tolerance under every
indexing mistake tried (test_attention_bias_dense).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1, 2], ids=["auto", "one_wg_per_item", "streamk_no_remap"], autouse=True)
def all_variants(request, hip):
    """Every kernel structure behind td_attention_bf16 must pass every case."""
    prev = hip.lib().td_attention_set_variant(request.param)
    yield
    hip.lib().td_attention_set_variant(prev)


def _ref(q, k, v, Hq, Hkv, causal):
    B, Sq, _ = q.shape
    Skv = k.shape[1]
    qh = q.float().reshape(B, Sq, Hq, 128).transpose(1, 2)
    kh = k.float().reshape(B, Skv, Hkv, 128).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    vh = v.float().reshape(B, Skv, Hkv, 128).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(128)
    if causal:
        i = torch.arange(Sq)[:, None] + (Skv - Sq)
        j = torch.arange(Skv)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    o = torch.softmax(s, dim=-1) @ vh
    return o.transpose(1, 2).reshape(B, Sq, Hq * 128)


def _check(got, ref, tol=2.0 ** -7):
    got = got.float().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max() / ref.abs().max()
    assert err < tol, f"rel-to-scale err {err:.3e}"


@pytest.mark.parametrize("S,H", [(64, 1), (256, 2), (449, 4), (1000, 3), (4289, 2)])
def test_joint_attention_inplace_qkv(hip, S, H):
    """FLUX layout: one [S, 3*H*128] projection buffer, q|k|v column blocks, output [S, H*128]."""
    g = torch.Generator().manual_seed(S + H)
    qkv = torch.randn(1, S, 3 * H * 128, generator=g).bfloat16()
    d = qkv.cuda()
    q, k, v = d[:, :, :H * 128], d[:, :, H * 128:2 * H * 128], d[:, :, 2 * H * 128:]
    out = torch.zeros(1, S, H * 128, dtype=torch.bfloat16, device="cuda")
    hip.attention(q, k, v, out, H, H)
    torch.cuda.synchronize()
    c = qkv
    _check(out, _ref(c[:, :, :H * 128], c[:, :, H * 128:2 * H * 128], c[:, :, 2 * H * 128:], H, H, False))


@pytest.mark.parametrize("B,S,H", [(1, 4289, 24), (1, 1000, 80), (2, 520, 50), (1, 4354, 24)])
def test_joint_attention_more_items_than_cus(hip, B, S, H):
    """More (query tile, head) items than CUs: the stream-K form (equal ranges of KV-tile iterations per persistent workgroup,
    items split across two workgroups merged through the hand-off workspace).  FLUX config 2 (S = 4289) and config 5 (S = 4354)
    shapes, a ragged 4-tile case and a batched one.  Run twice: the second launch finds the flags cleared by the first."""
    g = torch.Generator().manual_seed(S + H)
    qkv = torch.randn(B, S, 3 * H * 128, generator=g).bfloat16()
    d = qkv.cuda()
    q, k, v = d[:, :, :H * 128], d[:, :, H * 128:2 * H * 128], d[:, :, 2 * H * 128:]
    outs = []
    other = torch.randn(B, S, 3 * H * 128, generator=g).bfloat16().cuda()
    for i in range(3):
        out = torch.zeros(B, S, H * 128, dtype=torch.bfloat16, device="cuda")
        hip.attention(q, k, v, out, H, H)
        torch.cuda.synchronize()
        outs.append(out)
        if i == 1:
            # a launch on OTHER data in between: the LDS a workgroup finds then holds foreign tiles, so a read that runs ahead of its
            # LDS-DMA (a missing wait) cannot be masked by the previous launch's identical leftovers (round 3: the two-slot kernels
            # relied on a vmcnt(0) the compiler happened to place; repeated launches agreed with each other, the first one did not)
            hip.attention(other[:, :, :H * 128], other[:, :, H * 128:2 * H * 128], other[:, :, 2 * H * 128:], torch.empty_like(out), H, H)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    ref = torch.cat([_ref(qkv[:, :, h * 128:(h + 1) * 128], qkv[:, :, (H + h) * 128:(H + h + 1) * 128], qkv[:, :, (2 * H + h) * 128:(2 * H + h + 1) * 128], 1, 1, False)
                     for h in range(H)], dim=2)
    _check(outs[0], ref)


@pytest.mark.parametrize("shape", ["split_items", "one_tile_items"])
def test_stream_k_small_shapes(hip, shape):
    """The stream-K form at the smallest shapes that still take its two ways through an item, sized from the device's CU count:
    S = 300 with cus / 2 + 2 heads (two query tiles x five KV tiles per head, cus + 4 items: nearly every item is split over two
    workgroups and merged through the hand-off) and S = 64 with cus + 4 heads (one KV tile per item: nothing can be split, some
    workgroups run two items).  Within the module's tolerance of the fp32 reference; three launches with a foreign launch in between
    agree bit for bit; and variant 2 (no XCD remap) equals variant 0 bit for bit -- the ranges and the merge order of a split item
    do not depend on which physical workgroup takes a range."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    S, H = (300, cus // 2 + 2) if shape == "split_items" else (64, cus + 4)
    W = H * 128
    g = torch.Generator().manual_seed(S + H)
    qkv = torch.randn(1, S, 3 * W, generator=g).bfloat16()
    d = qkv.cuda()
    other = torch.randn(1, S, 3 * W, generator=g).bfloat16().cuda()

    def launch(x):
        out = torch.zeros(1, S, W, dtype=torch.bfloat16, device="cuda")
        hip.attention(x[:, :, :W], x[:, :, W:2 * W], x[:, :, 2 * W:], out, H, H)
        torch.cuda.synchronize()
        return out

    outs = [launch(d), launch(d)]
    launch(other)                                 # the LDS and the hand-off slots then hold foreign data
    outs.append(launch(d))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    _check(outs[0], _ref(qkv[:, :, :W], qkv[:, :, W:2 * W], qkv[:, :, 2 * W:], H, H, False))
    lib = hip.lib()
    cur = lib.td_attention_set_variant(2)
    try:
        if cur != 0:
            return                                # the module's fixture runs every variant: the 0-against-2 comparison is made once, under 0
        plain_order = launch(d)
    finally:
        lib.td_attention_set_variant(cur)
    assert torch.equal(outs[0], plain_order), "stream-K with and without the XCD remap differ"


def test_persistent_attention_concurrent_streams(hip):
    """Three persistent (stream-K) attention launches share the chip on three streams, many times over, beside an unrelated
    memory-bound kernel on a fourth: every result must equal the same launch run alone.  The split items' two owners never
    wait for each other (second arriver merges), so no residency or dispatch-order assumption is involved; each stream has its
    own hand-off workspace."""
    S, H, reps = 4289, 24, 12
    W = H * 128
    g = torch.Generator().manual_seed(77)
    ins = [torch.randn(1, S, 3 * W, generator=g).bfloat16().cuda() for _ in range(3)]
    alone = []
    for x in ins:
        o = torch.zeros(1, S, W, dtype=torch.bfloat16, device="cuda")
        hip.attention(x[:, :, :W], x[:, :, W:2 * W], x[:, :, 2 * W:], o, H, H)
        torch.cuda.synchronize()
        alone.append(o)
    streams = [torch.cuda.Stream() for _ in range(4)]
    noise = torch.empty(64 * 1024 * 1024, dtype=torch.bfloat16, device="cuda")
    outs = [[torch.zeros(1, S, W, dtype=torch.bfloat16, device="cuda") for _ in range(reps)] for _ in range(3)]
    torch.cuda.synchronize()
    for r in range(reps):
        for k in range(3):
            with torch.cuda.stream(streams[k]):
                x = ins[k]
                hip.attention(x[:, :, :W], x[:, :, W:2 * W], x[:, :, 2 * W:], outs[k][r], H, H)
        with torch.cuda.stream(streams[3]):
            noise.add_(1.0)                       # uneven load on the memory system while the hand-offs happen
    torch.cuda.synchronize()
    for k in range(3):
        for r in range(reps):
            assert torch.equal(outs[k][r], alone[k]), f"stream {k} repetition {r} differs from the launch run alone"


def test_attention_peaked_rows(hip):
    """Forces the online-softmax rescale: one key per row dominates late in the sequence."""
    g = torch.Generator().manual_seed(3)
    S, H = 512, 1
    q = torch.randn(1, S, 128, generator=g)
    k = torch.randn(1, S, 128, generator=g)
    v = torch.randn(1, S, 128, generator=g)
    k[0, 400] = q[0, 7] * 4.0      # row 7 spikes at key 400 (tile 6)
    k[0, 130] = q[0, 300] * 3.0    # row 300 spikes at key 130
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    out = torch.zeros(1, S, 128, dtype=torch.bfloat16, device="cuda")
    hip.attention(q.cuda(), k.cuda(), v.cuda(), out, 1, 1)
    torch.cuda.synchronize()
    _check(out, _ref(q, k, v, 1, 1, False))


@pytest.mark.parametrize("S,Hq,Hkv,B", [(300, 4, 2, 2), (1029, 28, 4, 1), (64, 2, 1, 1)])
def test_causal_gqa(hip, S, Hq, Hkv, B):
    """Qwen2-VL layout: fused [q(Hq)|k(Hkv)|v(Hkv)] projection, causal, grouped-query."""
    g = torch.Generator().manual_seed(S)
    W = (Hq + 2 * Hkv) * 128
    qkv = torch.randn(B, S, W, generator=g).bfloat16()
    d = qkv.cuda()
    sl = lambda t: (t[:, :, :Hq * 128], t[:, :, Hq * 128:(Hq + Hkv) * 128], t[:, :, (Hq + Hkv) * 128:])
    q, k, v = sl(d)
    out = torch.zeros(B, S, Hq * 128, dtype=torch.bfloat16, device="cuda")
    hip.attention(q, k, v, out, Hq, Hkv, causal=True)
    torch.cuda.synchronize()
    _check(out, _ref(*sl(qkv), Hq, Hkv, True))


def test_attention_strided_output(hip):
    """Single-block layout: attention output lands in columns [0, H*128) of the wider cat buffer."""
    g = torch.Generator().manual_seed(9)
    S, H = 300, 2
    qkv = torch.randn(1, S, 3 * H * 128, generator=g).bfloat16()
    d = qkv.cuda()
    cat = torch.zeros(1, S, H * 128 + 512, dtype=torch.bfloat16, device="cuda")
    hip.attention(d[:, :, :256], d[:, :, 256:512], d[:, :, 512:], cat[:, :, :H * 128], H, H)
    torch.cuda.synchronize()
    _check(cat[:, :, :H * 128], _ref(qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:], H, H, False))
    assert torch.count_nonzero(cat[:, :, H * 128:]) == 0


def test_packed_variable_length_segments(hip):
    """td_attention_varlen_bf16 (the vision towers' cu_seqlens): one launch over packed segments of very different lengths
    equals full attention run inside each segment on its own; nothing leaks across segment borders."""
    H = 2
    lens = [300, 1, 64, 257, 880, 31]
    S = sum(lens)
    g = torch.Generator().manual_seed(21)
    qkv = torch.randn(S, 3 * H * 128, generator=g).bfloat16()
    d = qkv.cuda()
    starts = torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32).cuda()
    out = hip.attention_padded_varlen(d, H, 128 ** -0.5, starts, max(lens))
    torch.cuda.synchronize()
    W = H * 128
    r0 = 0
    for n in lens:
        c = qkv[r0:r0 + n][None]
        ref = _ref(c[:, :, :W], c[:, :, W:2 * W], c[:, :, 2 * W:], H, H, False)
        _check(out[r0:r0 + n][None], ref)
        alone = hip.attention_padded(d[r0:r0 + n], H, 128 ** -0.5)
        torch.cuda.synchronize()
        assert _rel_close(out[r0:r0 + n], alone)
        r0 += n


def _rel_close(a, b, tol=2.0 ** -7):
    a, b = a.float().cpu(), b.float().cpu()
    return bool((a - b).abs().max() <= tol * b.abs().max())


@pytest.mark.parametrize("S,H", [(449, 4), (4289, 24), (1000, 80)])
def test_fixed_reference_point_form(hip, S, H):
    """td_attention_joint_prescaled_bf16 with a score bound: the scores are exponentiated as they are, no reference point at all (what the FLUX
    engine does with the bound its QK-RMSNorm weights give).  Same answer as the running-maximum form to the bf16 rounding of the probabilities,
    whether the bound is the Cauchy-Schwarz one, the largest admitted (48 octaves), or too LOW by two octaves (a score above it is harmless)."""
    g = torch.Generator().manual_seed(S * 5 + H)
    qkv = torch.randn(S, 3 * H * 128, generator=g).bfloat16()
    c = (128 ** -0.5) * 1.4426950408889634
    qkv[:, :H * 128] = (qkv[:, :H * 128].float() * c).bfloat16()
    d = qkv.cuda()
    q, k, v = d[:, :H * 128], d[:, H * 128:2 * H * 128], d[:, 2 * H * 128:]
    qh, kh = qkv[:, :H * 128].float().view(S, H, 128), qkv[:, H * 128:2 * H * 128].float().view(S, H, 128)
    cs = float((qh.norm(dim=2).amax() * kh.norm(dim=2).amax()))              # Cauchy-Schwarz over all rows and heads
    smax = max(float((qh[:, h] @ kh[:, h].T).amax()) for h in ([0, H - 1] if H > 4 else range(H)))
    base = hip.attention_joint_prescaled(q, k, v, torch.zeros(S, H * 128, dtype=torch.bfloat16, device="cuda"), H, 0.0)
    torch.cuda.synchronize()
    assert torch.isfinite(base.float()).all()
    for bound in (cs, 48.0, max(smax - 2.0, 0.5)):
        out = hip.attention_joint_prescaled(q, k, v, torch.zeros(S, H * 128, dtype=torch.bfloat16, device="cuda"), H, bound)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
        _check(out, base.float().cpu(), 2.0 ** -7)
    hs = [0, H - 1] if H > 4 else list(range(H))
    for h in hs:
        ref = torch.softmax((qh[:, h] @ kh[:, h].T) * math.log(2.0), dim=-1) @ qkv[:, (2 * H + h) * 128:(2 * H + h + 1) * 128].float()
        _check(out[:, h * 128:(h + 1) * 128], ref)
    with pytest.raises(hip.ThinkDiffHipError):
        hip.attention_joint_prescaled(q, k, v, torch.zeros(S, H * 128, dtype=torch.bfloat16, device="cuda"), H, 49.0)


@pytest.mark.parametrize("S,H", [(449, 4), (4289, 24), (4354, 24)])
def test_prescaled_q_form(hip, S, H):
    """The form the FLUX engine uses: q arrives multiplied by scale * log2(e) (rounded to bf16 once, where RoPE rounds it), the
    kernel applies no scale of its own and exponentiates in base 2.  Reference: softmax over ln(2) * q'.k in fp32."""
    g = torch.Generator().manual_seed(S * 3 + H)
    qkv = torch.randn(1, S, 3 * H * 128, generator=g).bfloat16()
    c = (128 ** -0.5) * 1.4426950408889634
    qkv[:, :, :H * 128] = (qkv[:, :, :H * 128].float() * c).bfloat16()
    d = qkv.cuda()
    q, k, v = d[:, :, :H * 128], d[:, :, H * 128:2 * H * 128], d[:, :, 2 * H * 128:]
    lib = hip.lib()
    cur = lib.td_attention_set_variant(0)
    lib.td_attention_set_variant(cur | 0x800)
    try:
        out = torch.zeros(1, S, H * 128, dtype=torch.bfloat16, device="cuda")
        hip.attention(q, k, v, out, H, H)
        torch.cuda.synchronize()
    finally:
        lib.td_attention_set_variant(cur)
    hs = [0, H - 1] if H > 4 else list(range(H))              # the fp32 reference of 24 heads x 4354^2 is slow: check two heads
    for h in hs:
        qh = qkv[0, :, h * 128:(h + 1) * 128].float()
        kh = qkv[0, :, (H + h) * 128:(H + h + 1) * 128].float()
        vh = qkv[0, :, (2 * H + h) * 128:(2 * H + h + 1) * 128].float()
        ref = torch.softmax((qh @ kh.T) * math.log(2.0), dim=-1) @ vh
        _check(out[0, :, h * 128:(h + 1) * 128], ref)


@pytest.mark.parametrize("form", ["joint_running_max", "joint_prescaled_no_bound", "causal_gqa"])
def test_running_maximum_forms_never_miss_a_score(hip, form):
    """The running-maximum softmax (no score bound: norm-weight products above ~2.9, the stand-alone entry, every causal / GQA kernel) on LARGE inputs with
    scores up to +-60 octaves: 2.5 M rows, every output element finite and every row a convex combination of its values.  A row maximum that missed an
    element -- the first read of fresh QK^T accumulators being an inline-asm v_max3 the compiler's hazard recogniser cannot see (csrc/attention_common.h;
    the e4m3 kernel met it as one NaN row in ~600) -- shows up here as inf / NaN or as an output outside the value range."""
    g = torch.Generator(device="cuda").manual_seed(11)
    if form == "causal_gqa":
        B, S, Hq, Hkv = 2, 3000, 28, 4
        q = (torch.randn(B, S, Hq * 128, generator=g, device="cuda") * 2.5).bfloat16()
        k = (torch.randn(B, S, Hkv * 128, generator=g, device="cuda") * 2.5).bfloat16()
        v = torch.rand(B, S, Hkv * 128, generator=g, device="cuda").bfloat16()
        out = torch.empty(B, S, Hq * 128, dtype=torch.bfloat16, device="cuda")
        for _ in range(3):
            hip.attention(q, k, v, out, Hq, Hkv, causal=True)
    else:
        S, H = 4354, 24
        q = (torch.randn(S, H * 128, generator=g, device="cuda") * 2.5).bfloat16()
        k = (torch.randn(S, H * 128, generator=g, device="cuda") * 2.5).bfloat16()
        v = torch.rand(S, H * 128, generator=g, device="cuda").bfloat16()
        out = torch.empty(S, H * 128, dtype=torch.bfloat16, device="cuda")
        for _ in range(3):
            if form == "joint_running_max":
                hip.attention(q[None], k[None], v[None], out[None], H, H)
            else:
                hip.attention_joint_prescaled((q.float() * (128 ** -0.5 * 1.4426950408889634)).bfloat16(), k, v, out, H, score_bound=0.0)
    torch.cuda.synchronize()
    o = out.float()
    assert torch.isfinite(o).all()
    assert float(o.min()) >= -1e-3 and float(o.max()) <= 1.0 + 2.0 ** -7      # values lie in [0, 1): so does every probability-weighted mean of them


# ---- causal attention against a KV cache: decode (Sq = 1) and cached prefill (1 < Sq < Skv) ------------------------------

def _ref64(q, k, v, Hq, Hkv):
    """float64 causal attention of the last Sq positions against Skv keys (query i sees keys j <= i + Skv - Sq)."""
    B, Sq, _ = q.shape
    Skv = k.shape[1]
    qh = q.double().reshape(B, Sq, Hq, 128).transpose(1, 2)
    kh = k.double().reshape(B, Skv, Hkv, 128).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    vh = v.double().reshape(B, Skv, Hkv, 128).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(128)
    i = torch.arange(Sq)[:, None] + (Skv - Sq)
    s = s.masked_fill(torch.arange(Skv)[None, :] > i, float("-inf"))
    o = torch.softmax(s, dim=-1) @ vh
    return o.transpose(1, 2).reshape(B, Sq, Hq * 128)


def _cache(B, Skv, Hkv, g, vmode, dom, q):
    """k, v [B, max_len, Hkv*128] views into one cache-shaped buffer (k | v | pad columns, max_len > Skv rows, the rows past Skv
    filled with large values that must not be read).  vmode: 'randn', 'big' (|v| up to 1e3) or 'offset' (a common offset of 500).
    dom: None or the key index made dominant for every q head of its kv head."""
    max_len, ld = Skv + 7, 2 * Hkv * 128 + 64
    buf = torch.randn(B, max_len, ld, generator=g)
    Hq = q.shape[2] // 128
    if vmode == "big":
        buf[:, :, Hkv * 128:2 * Hkv * 128] *= 330.0
        buf[:, :, Hkv * 128:2 * Hkv * 128].clamp_(-1000.0, 1000.0)
    elif vmode == "offset":
        buf[:, :, Hkv * 128:2 * Hkv * 128] += 500.0
    if dom is not None:
        qg = q.float().reshape(B, Hq, 128).reshape(B, Hkv, Hq // Hkv, 128).sum(dim=2)      # [B, Hkv, 128]
        buf[:, dom, :Hkv * 128] = 3.0 * qg.reshape(B, Hkv * 128)
    buf[:, Skv:, :] = 1e4                 # rows past the sequence: would dominate every score / value if read
    buf = buf.bfloat16()
    return buf, buf[:, :Skv, :Hkv * 128], buf[:, :Skv, Hkv * 128:2 * Hkv * 128]


# (Hq, Hkv, Skv, batch, dominant key, v mode): every value of every axis at least once; the long caches with small batches
DECODE_CASES = [
    (12, 2, 1, 70, None, "randn"), (28, 4, 2, 3, "last_key", "big"), (4, 4, 15, 3, "first", "offset"), (7, 1, 16, 70, "last_slot", "randn"),
    (12, 2, 17, 3, "last_key", "big"), (28, 4, 63, 1, "first", "randn"), (7, 1, 64, 3, "last_slot", "offset"), (4, 4, 65, 70, "last_key", "randn"),
    (12, 2, 300, 70, None, "big"), (28, 4, 300, 70, "last_slot", "randn"), (28, 4, 1025, 3, "last_key", "offset"), (7, 1, 8192, 1, "first", "big"),
    (12, 2, 8192, 1, "last_slot", "randn"),
]


@pytest.mark.parametrize("Hq,Hkv,Skv,B,dom,vmode", DECODE_CASES)
def test_decode_against_cache(hip, request, Hq, Hkv, Skv, B, dom, vmode):
    """Sq = 1, causal through hip.attention: td_attention_bf16 routes it to the decode kernel (csrc/attention_decode.hip: 16 key slots
    over 4 waves, fp32 softmax and accumulation) under 'auto', to the tile kernel under the other variants.  k / v are read from a
    cache-shaped buffer (batch stride max_len x ld with max_len > Skv).  Every forced q-head group that divides Hq / Hkv runs, and the
    automatic choice; a second launch must give identical bits.

    Bound under 'auto' (P stays fp32): |err| <= 1 bf16 ulp of the reference + 2^-12 max |v| of the kv head (the fp32 softmax
    weights carry ~1e-6 relative error, which the value offset / magnitude scales).  Under variants 1 / 2 the tile kernel rounds P
    to bf16: the module's 2^-7 of the output scale."""
    variant = request.node.callspec.params["all_variants"]
    g = torch.Generator().manual_seed(Skv * 131 + B * 7 + Hq)
    q = torch.randn(B, 1, Hq * 128, generator=g).bfloat16()
    qbuf = torch.zeros(B, 1, Hq * 128 + 64, dtype=torch.bfloat16)
    qbuf[:, :, :Hq * 128] = q
    pos = {None: None, "first": 0, "last_slot": min(15, Skv - 1), "last_key": Skv - 1}[dom]
    buf, k, v = _cache(B, Skv, Hkv, g, vmode, pos, q)
    ref = _ref64(q, k, v, Hq, Hkv)
    dbuf = buf.cuda()
    dk, dv = dbuf[:, :Skv, :Hkv * 128], dbuf[:, :Skv, Hkv * 128:2 * Hkv * 128]
    dq = qbuf.cuda()[:, :, :Hq * 128]
    groups = [0] + [gg for gg in (1, 2, 3, 4, 6, 7) if (Hq // Hkv) % gg == 0] if variant == 0 else [0]
    vmax = v.double().abs().reshape(B, 1, Skv, Hkv, 128).amax(dim=(2, 4))                                # [B, 1, Hkv]
    vmax = vmax.repeat_interleave(Hq // Hkv * 128, dim=2)                                               # [B, 1, Hq*128]
    worst = 0.0
    for grp in groups:
        prev = hip.lib().td_attention_decode_set_group(grp)
        try:
            outs = []
            for _ in range(2):
                out = torch.full((B, 1, Hq * 128), -7.0, dtype=torch.bfloat16, device="cuda")
                hip.attention(dq, dk, dv, out, Hq, Hkv, causal=True)
                outs.append(out)
            torch.cuda.synchronize()
        finally:
            hip.lib().td_attention_decode_set_group(prev)
        assert torch.equal(outs[0], outs[1]), f"group {grp}: a repeated launch gave different bits"
        got = outs[0].double().cpu()
        assert torch.isfinite(got).all()
        if variant == 0:
            a = ref.abs().clamp_min(2.0 ** -126)
            tol = torch.exp2(torch.floor(torch.log2(a)) - 7) + 2.0 ** -12 * vmax
            r = ((got - ref).abs() / tol).max().item()
            worst = max(worst, r)
            assert r <= 1.0, f"group {grp}: max error {r:.3g} x the bound"
        else:
            worst = max(worst, ((got - ref).abs().max() / ref.abs().max()).item() / 2.0 ** -7)
            _check(outs[0], ref)
    print(f"decode variant {variant} Hq={Hq} Hkv={Hkv} Skv={Skv} B={B}: max error {worst:.3f} x the bound")


@pytest.mark.parametrize("Sq,Skv", [(2, 300), (17, 64), (256, 1029), (300, 4096)])
def test_cached_prefill_causal_gqa(hip, Sq, Skv):
    """1 < Sq < Skv, causal, GQA: a prefill chunk against a longer cache (query i sees keys j <= i + Skv - Sq), batch 2, k / v from a
    cache-shaped buffer.  float64 masked softmax reference; the module's tolerance (2^-7 of the output scale)."""
    B, Hq, Hkv = 2, 12, 2
    g = torch.Generator().manual_seed(Sq * 13 + Skv)
    q = torch.randn(B, Sq, Hq * 128, generator=g).bfloat16()
    buf, k, v = _cache(B, Skv, Hkv, g, "randn", None, q[:, :1])
    ref = _ref64(q, k, v, Hq, Hkv)
    dbuf = buf.cuda()
    out = torch.full((B, Sq, Hq * 128), -7.0, dtype=torch.bfloat16, device="cuda")
    hip.attention(q.cuda(), dbuf[:, :Skv, :Hkv * 128], dbuf[:, :Skv, Hkv * 128:2 * Hkv * 128], out, Hq, Hkv, causal=True)
    torch.cuda.synchronize()
    print(f"cached prefill Sq={Sq} Skv={Skv}: max error {((out.double().cpu() - ref).abs().max() / ref.abs().max()).item() / 2.0 ** -7:.3f} x the bound")
    _check(out, ref)


# ---- score-bias attention (td_attention_bias_bf16: the BIAS instantiations of the tile kernel) ---------------------------

def _ref64_bias(q, k, v, Hq, Hkv, scale, causal, bias):
    """float64 softmax(q.k^T * scale + bias [+ causal mask, query i sees keys j <= i + Skv - Sq]) . v of 2-D operands
    q [Sq, Hq*128], k / v [Skv, Hkv*128], bias [Hq, Sq, Skv] -> [Sq, Hq*128]."""
    Sq, Skv = q.shape[0], k.shape[0]
    qh = q.double().reshape(Sq, Hq, 128).transpose(0, 1)
    kh = k.double().reshape(Skv, Hkv, 128).transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
    vh = v.double().reshape(Skv, Hkv, 128).transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
    s = qh @ kh.transpose(-1, -2) * scale + bias.double()
    if causal:
        i = torch.arange(Sq)[:, None] + (Skv - Sq)
        s = s.masked_fill(torch.arange(Skv)[None, :] > i, float("-inf"))
    o = torch.softmax(s, dim=-1) @ vh
    return o.transpose(0, 1).reshape(Sq, Hq * 128)


def _check_bias(got, ref, what):
    """The module's bar (_check: |err| <= 2^-7 max|ref|), with the figure and the worst element printed first."""
    g = got.double().cpu()
    err = (g - ref).abs()
    i = int(torch.argmax(err))
    r, c = divmod(i, ref.shape[1])
    print(f"{what}: max error {float(err.max() / ref.abs().max()) / 2.0 ** -7:.3f} x the bound (row {r} col {c}: got {float(g[r, c]):.6g} "
          f"ref {float(ref[r, c]):.6g})")
    _check(got, ref)


SCALE_D = 128 ** -0.5
# (Sq, Skv, Hq, Hkv, scale, causal): the smallest shapes that reach every branch of the BIAS tile body (64-key tile, 32 query rows per
# wave, 256 per workgroup, one float4 of bias per 4 keys): a 36-key last tile (the `kbase + 4 <= Skv` guard splits an 8-key group);
# GQA + inv_scale + Sq % 32 != 0 (the qrow clamp); a second query workgroup of 44 rows; causal with bias, offset 0 and 64; Sq = 1
# (with a bias this must stay on the tile kernel, not the decode kernel)
BIAS_CASES = [(100, 100, 3, 3, 1.0, False), (45, 132, 4, 2, SCALE_D, False), (300, 68, 2, 2, SCALE_D, False),
              (76, 76, 2, 2, 1.0, True), (40, 104, 2, 1, SCALE_D, True), (1, 68, 2, 2, SCALE_D, True)]
_bias_cache = {}


def _bias_case(Sq, Skv, Hq, Hkv, scale, causal):
    """Operands, fp64 reference and the CPU mutation margins of one dense case (computed once, shared by the kernel variants).
    bias: fp32 randn of std 2, independent per (head, row, key) -- not Toeplitz, so a read that is a key, a row or a head off
    changes it completely; for scale = 1 q and k are scaled by 0.3 so that q.k (std ~1) and the bias both matter."""
    key = (Sq, Skv, Hq, Hkv, scale, causal)
    if key not in _bias_cache:
        g = torch.Generator().manual_seed(Sq * 1009 + Skv * 31 + Hq)
        amp = 0.3 if scale == 1.0 else 1.0
        q = (torch.randn(Sq, Hq * 128, generator=g) * amp).bfloat16()
        k = (torch.randn(Skv, Hkv * 128, generator=g) * amp).bfloat16()
        v = torch.randn(Skv, Hkv * 128, generator=g).bfloat16()
        bias = torch.randn(Hq, Sq, Skv, generator=g) * 2.0
        ref = _ref64_bias(q, k, v, Hq, Hkv, scale, causal, bias)
        mutants = {"rolled by one key": torch.roll(bias, 1, dims=2), "rolled by four keys": torch.roll(bias, 4, dims=2)}
        if Sq > 1:
            mutants["rolled by one row"] = torch.roll(bias, 1, dims=1)
        if Hq > 1:
            mutants["rolled by one head"] = torch.roll(bias, 1, dims=0)
        if Skv % 64:
            z = bias.clone()
            z[:, :, Skv // 64 * 64:] = 0.0
            mutants["zeroed on the ragged last tile"] = z
        if scale != 1.0:
            mutants["bias * scale"] = bias * scale
        margins = {name: float((_ref64_bias(q, k, v, Hq, Hkv, scale, causal, b) - ref).abs().max() / ref.abs().max()) / 2.0 ** -7
                   for name, b in mutants.items()}
        _bias_cache[key] = (q, k, v, bias, ref, margins)
    return _bias_cache[key]


@pytest.mark.parametrize("Sq,Skv,Hq,Hkv,scale,causal", BIAS_CASES)
def test_attention_bias_dense(hip, Sq, Skv, Hq, Hkv, scale, causal):
    """td_attention_bias_bf16 with a dense random bias against float64.  First a condition on the INPUTS: the fp64 reference recomputed
    with each plausible indexing mistake (bias a key, four keys, a row or a head off, dropped on the ragged last tile, multiplied by
    scale instead of added as it is) lies >= 10x the tolerance from the true one, so the kernel cannot pass with any of them.
    Measured margins (fp64, CPU; x the 2^-7 tolerance), smallest mutant of each case: 100x100 131; 45x132 58; 300x68 94; 76x76 causal 83;
    40x104 causal 83; 1x68 causal 44 (the smallest is always the bias dropped on the ragged last tile; the rolls and bias * scale lie
    at 115 - 300).  Kernel on MI355X, max error x the bound, the same under all three variants: 0.30, 0.31, 0.36, 0.24, 0.40, 0.43."""
    q, k, v, bias, ref, margins = _bias_case(Sq, Skv, Hq, Hkv, scale, causal)
    for name, m in margins.items():
        print(f"bias {Sq}x{Skv} Hq={Hq} causal={causal}: mutant '{name}' lies {m:.1f} x the tolerance from the reference")
        assert m >= 10.0, f"inputs too weak: mutant '{name}' only {m:.2f} x the tolerance away"
    out = torch.full((Sq, Hq * 128), -7.0, dtype=torch.bfloat16, device="cuda")
    hip.attention_bias(q.cuda(), k.cuda(), v.cuda(), out, Hq, Hkv, scale, causal, bias.cuda())
    torch.cuda.synchronize()
    _check_bias(out, ref, f"bias attention {Sq}x{Skv} Hq={Hq} Hkv={Hkv} scale={scale:.4f} causal={causal}")


@pytest.mark.parametrize("scale", [1.0, SCALE_D])
def test_attention_bias_carrying_a_mask(hip, scale):
    """A bias that carries a mask, as T5 and the vision towers use it: -1e4 on ALL keys of the first tile for rows >= 10 (the first tile
    sets the reference point of the row's exponentials at about -1e4 / scale; the next tile must move it by that much and wipe
    what the first one accumulated) and on a random 30 % of the other keys, on top of the random bias.  Sq = Skv = 132.
    Measured on MI355X: max error 0.33 (scale 1) and 0.42 (scale 128^-0.5) x the bound."""
    S, H = 132, 2
    g = torch.Generator().manual_seed(132)
    amp = 0.3 if scale == 1.0 else 1.0
    q = (torch.randn(S, H * 128, generator=g) * amp).bfloat16()
    k = (torch.randn(S, H * 128, generator=g) * amp).bfloat16()
    v = torch.randn(S, H * 128, generator=g).bfloat16()
    bias = torch.randn(H, S, S, generator=g) * 2.0
    block = torch.zeros(H, S, S, dtype=torch.bool)
    block[:, 10:, :64] = True
    masked = block | ((torch.rand(H, S, S, generator=g) < 0.3) & ~block)
    assert (~masked).any(dim=2).all()
    bias = bias + masked.float() * -1e4
    ref = _ref64_bias(q, k, v, H, H, scale, False, bias)
    out = torch.full((S, H * 128), -7.0, dtype=torch.bfloat16, device="cuda")
    hip.attention_bias(q.cuda(), k.cuda(), v.cuda(), out, H, H, scale, False, bias.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    _check_bias(out, ref, f"bias attention with a -1e4 mask, scale={scale:.4f}")


def test_attention_bias_late_spike(hip):
    """+40 at one key of the third tile for a few rows (Skv = 200): the online softmax must move its reference point because of the
    BIAS (q.k * scale stays within a few units), and those rows become that key's value row.  Measured on MI355X: 0.34 x the bound."""
    Sq, Skv, H, key = 70, 200, 2, 150
    rows = [3, 40, 69]
    g = torch.Generator().manual_seed(200)
    q = torch.randn(Sq, H * 128, generator=g).bfloat16()
    k = torch.randn(Skv, H * 128, generator=g).bfloat16()
    v = torch.randn(Skv, H * 128, generator=g).bfloat16()
    bias = torch.randn(H, Sq, Skv, generator=g) * 2.0
    bias[:, rows, key] += 40.0
    assert float((q.double().view(Sq, H, 128).transpose(0, 1) @ k.double().view(Skv, H, 128).transpose(0, 1).transpose(1, 2)).abs().max()) * SCALE_D < 8.0
    ref = _ref64_bias(q, k, v, H, H, SCALE_D, False, bias)
    assert (ref[rows] - v[key].double()).abs().max() < 1e-6          # the spike owns those rows: only the bias can have done that
    out = torch.full((Sq, H * 128), -7.0, dtype=torch.bfloat16, device="cuda")
    hip.attention_bias(q.cuda(), k.cuda(), v.cuda(), out, H, H, SCALE_D, False, bias.cuda())
    torch.cuda.synchronize()
    _check_bias(out, ref, "bias attention with a +40 spike in the third tile")


@pytest.mark.parametrize("causal", [False, True])
def test_attention_zero_bias_is_the_plain_kernel(hip, causal):
    """An all-zero bias on a shape with fewer (query tile, head) items than CUs (so td_attention_bf16 takes the tile kernel too, not
    stream-K): bit-identical to hip.attention on the same operands -- st + 0 * inv_scale is exact, so any difference means the BIAS
    and the plain instantiations of the tile kernel have diverged."""
    S, H = 300, 2
    g = torch.Generator().manual_seed(300 + causal)
    qkv = torch.randn(S, 3 * H * 128, generator=g).bfloat16().cuda()
    q, k, v = qkv[:, :H * 128], qkv[:, H * 128:2 * H * 128], qkv[:, 2 * H * 128:]
    plain = torch.full((1, S, H * 128), -7.0, dtype=torch.bfloat16, device="cuda")
    hip.attention(q[None], k[None], v[None], plain, H, H, scale=SCALE_D, causal=causal)
    out = torch.full((S, H * 128), 5.0, dtype=torch.bfloat16, device="cuda")
    hip.attention_bias(q, k, v, out, H, H, SCALE_D, causal, torch.zeros(H, S, S, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(out, plain[0])


@pytest.mark.parametrize("pad", [64, 4])
def test_attention_bias_strided_operands(hip, pad):
    """q, k, v as column slices of ONE fused [S, (Hq + 2 Hkv) * 128 + 64] buffer (the T5 layout), out into a wider buffer pre-filled with
    a sentinel: the pad columns of out stay untouched.  pad = 4: rows of out are 8- but not 16-byte aligned (the narrow store form).
    Measured on MI355X: max error 0.33 (pad 64) and 0.38 (pad 4) x the bound."""
    S, Hq, Hkv = 100, 4, 2
    g = torch.Generator().manual_seed(7 + pad)
    W = (Hq + 2 * Hkv) * 128
    buf = torch.randn(S, W + 64, generator=g).bfloat16()
    bias = torch.randn(Hq, S, S, generator=g) * 2.0
    sl = lambda t: (t[:, :Hq * 128], t[:, Hq * 128:(Hq + Hkv) * 128], t[:, (Hq + Hkv) * 128:W])
    ref = _ref64_bias(*sl(buf), Hq, Hkv, SCALE_D, False, bias)
    wide = torch.full((S, Hq * 128 + pad), -7.0, dtype=torch.bfloat16, device="cuda")
    hip.attention_bias(*sl(buf.cuda()), wide[:, :Hq * 128], Hq, Hkv, SCALE_D, False, bias.cuda())
    torch.cuda.synchronize()
    _check_bias(wide[:, :Hq * 128], ref, f"bias attention, strided operands, out pad {pad}")
    assert (wide[:, Hq * 128:].float() == -7.0).all(), "pad columns of out written"


def test_attention_bias_refusals(hip):
    """Skv % 4 != 0 (the float4 bias loads would straddle rows) and a bias pointer that is not 16-byte aligned: TD_ERR_INVALID before
    any launch, out unchanged."""
    H = 2
    for Sq, Skv, shift in [(16, 70, 0), (16, 68, 1)]:
        q = torch.randn(Sq, H * 128).bfloat16().cuda()
        k = torch.randn(Skv, H * 128).bfloat16().cuda()
        v = torch.randn(Skv, H * 128).bfloat16().cuda()
        flat = torch.zeros(H * Sq * Skv + 4, dtype=torch.float32, device="cuda")
        bias = flat[shift:shift + H * Sq * Skv].view(H, Sq, Skv)
        assert bias.data_ptr() % 16 == 4 * shift
        out = torch.full((Sq, H * 128), -7.0, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(hip.ThinkDiffHipError, match="error 2"):
            hip.attention_bias(q, k, v, out, H, H, SCALE_D, False, bias)
        torch.cuda.synchronize()
        assert (out.float() == -7.0).all()
