"""The e4m3 KV cache of the Qwen2-VL decode engine on the GPU: the row quantiser and dequantiser bit for bit against the CPU restatement
(tests/qwen2_kv8_common.py), the decode attention over bytes + scales against float64 over the dequantised cache, and the engine / get_embed with
the 8-bit cache against a restatement of the oracle's decoder loop that rounds every new k, v through the format before anybody reads it.

The model under test is an ordinary bf16 model whose cache holds K^ | V^ (x^ is a bf16 value exactly), so the attention bound is the bf16 decode
kernel's (tests/test_attention_gpu.py::test_decode_against_cache) and the engine bars are those of
tests/test_qwen2_w8_gpu.py::test_engine_decode_with_quantised_weights against the same pair of references.
"""
import ctypes
import functools

import pytest
import torch

import qwen2_kv8_common as K
import qwen2_w8_common as W
from oracle import qwen2vl_ref as Q

pytestmark = pytest.mark.gpu


def _ops():
    from thinkdiff.ops import register
    return register()          # torch.ops.thinkdiff_hip, loaded on first use


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


# ---- 1. quantiser and dequantiser -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 5, 300])
@pytest.mark.parametrize("heads", [2, 4, 8])
def test_kv_quantiser_bit_for_bit(hip, rows, heads):
    """Bytes, scales and kv_hat against the restatement on the corner-case vectors; dst_rows a permutation into larger planes (pad columns, more rows) whose
    other rows and columns must stay untouched; kv_hat aliased with kv; the identity row map; the torch op."""
    x = K.edge_kv_rows(rows, heads, seed=17 * rows + heads)
    q_ref, s_ref, hat_ref, _ = K.quantize_kv_rows(x, heads)
    R, W8, WS = rows + 9, heads * 128 + 64, heads + 3
    g = torch.Generator().manual_seed(rows)
    dst = torch.randperm(R, generator=g)[:rows].to(torch.int32)
    src = torch.zeros(rows, heads * 128 + 8, dtype=torch.bfloat16)      # (a row stride above the width)
    src[:, :heads * 128] = x
    xd = src.cuda()[:, :heads * 128]
    qbuf = torch.full((R, W8), 0xA5, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((R, WS), -3.0, dtype=torch.float32, device="cuda")
    q, s, hat = hip.kv_quant_rows_e4m3(xd, heads, q=qbuf, scale=sbuf, dst_rows=dst.cuda())
    torch.cuda.synchronize()
    qc, sc = qbuf.cpu(), sbuf.cpu()
    assert torch.equal(qc[dst.long(), :heads * 128], q_ref), "bytes"
    assert torch.equal(sc[dst.long(), :heads], s_ref), "scales"
    assert torch.equal(hat.float().cpu(), hat_ref), "kv_hat"
    assert torch.equal(xd.cpu(), x), "the source rows moved without inplace"
    others = torch.ones(R, dtype=torch.bool)
    others[dst.long()] = False
    assert bool((qc[others] == 0xA5).all()) and bool((qc[:, heads * 128:] == 0xA5).all()), "bytes outside the named rows / columns were written"
    assert bool((sc[others] == -3.0).all()) and bool((sc[:, heads:] == -3.0).all()), "scales outside the named rows / columns were written"
    # identity row map, aliased kv_hat
    q2, s2, hat2 = hip.kv_quant_rows_e4m3(xd, heads, inplace=True)
    torch.cuda.synchronize()
    assert hat2.data_ptr() == xd.data_ptr()
    assert torch.equal(q2.cpu(), q_ref) and torch.equal(s2.cpu(), s_ref) and torch.equal(xd.float().cpu(), hat_ref)
    # quantise -> dequantise -> quantise: what the restatement gives for x^ (the same bytes, or the exponent one lower with doubled bytes), x^ itself unmoved
    back = hip.kv_dequant_rows_e4m3(q2, s2)
    q3, s3, hat3 = hip.kv_quant_rows_e4m3(back, heads)
    torch.cuda.synchronize()
    assert torch.equal(back.float().cpu(), hat_ref), "dequantiser"
    q3_ref, s3_ref, hat3_ref, _ = K.quantize_kv_rows(hat_ref, heads)
    assert torch.equal(q3.cpu(), q3_ref) and torch.equal(s3.cpu(), s3_ref) and torch.equal(hat3.float().cpu(), hat_ref) and torch.equal(hat3_ref, hat_ref)
    same = (s3_ref == s_ref).repeat_interleave(128, dim=1)
    assert torch.equal(q3.cpu()[same], q_ref[same]) and float(same.float().mean()) > 0.5
    # strided planes into the dequantiser; the torch ops
    assert torch.equal(hip.kv_dequant_rows_e4m3(qbuf[dst.long().cuda()][:, :heads * 128], sbuf[dst.long().cuda()][:, :heads].contiguous()).float().cpu(), hat_ref)
    x2 = x.cuda()
    qo, so, ho = _ops().kv_quant_rows_e4m3(x2, heads)
    bo = _ops().kv_dequant_rows_e4m3(qo, so)
    torch.cuda.synchronize()
    assert torch.equal(qo.cpu(), q_ref) and torch.equal(so.cpu(), s_ref) and torch.equal(ho.float().cpu(), hat_ref) and torch.equal(bo.float().cpu(), hat_ref)


# ---- 2. the decode attention ------------------------------------------------------------------------------------------------------------------
def _device_planes(case):
    """The case's planes inside cache-shaped buffers: pad columns, max_len > Skv rows; every byte that must not be read is 0x7F (e4m3 NaN) and every scale
    that must not be read 2^40 -- the rows past each sequence's length included -- so a read past the end shows."""
    B, Skv, Hkv = case["B"], case["Skv"], case["Hkv"]
    max_len, ldkv, lds = Skv + 7, 2 * Hkv * 128 + 64, 2 * Hkv + 3
    qb = torch.full((B, max_len, ldkv), 0x7F, dtype=torch.uint8)
    sb = torch.full((B, max_len, lds), 2.0 ** 40, dtype=torch.float32)
    for b, n in enumerate(case["lens"]):
        qb[b, :n, :2 * Hkv * 128] = case["bytes"][b, :n]
        sb[b, :n, :2 * Hkv] = case["scale"][b, :n]
    qb, sb = qb.cuda(), sb.cuda()
    return qb[:, :Skv, :Hkv * 128], qb[:, :Skv, Hkv * 128:2 * Hkv * 128], sb[:, :Skv, :Hkv], sb[:, :Skv, Hkv:2 * Hkv]


def _run_decode8(hip, case, uncovered, what, use_lens):
    Hq, Hkv, B = case["Hq"], case["Hkv"], case["B"]
    ref, vmax = K.attention_ref64(case)
    tol = K.attention_tol(ref, vmax)
    K.check_mutant_margins(case, ref, tol, uncovered, what)          # the condition on the inputs, on the CPU, before any launch
    k8, v8, ks, vs = _device_planes(case)
    qbuf = torch.zeros(B, Hq * 128 + 64, dtype=torch.bfloat16)
    qbuf[:, :Hq * 128] = case["q"]
    dq = qbuf.cuda()[:, :Hq * 128]
    lens = torch.tensor(case["lens"], dtype=torch.int32).cuda() if use_lens else None
    worst = 0.0
    for grp in [0] + [gg for gg in (1, 2, 3, 4, 6, 7) if (Hq // Hkv) % gg == 0]:
        prev = hip.lib().td_attention_decode_set_group(grp)
        try:
            outs = []
            for _ in range(2):
                out = torch.full((B, Hq * 128), -7.0, dtype=torch.bfloat16, device="cuda")
                hip.attention_decode_kv8(dq, k8, v8, ks, vs, Hq, Hkv, kv_lens=lens, out=out)
                outs.append(out)
            torch.cuda.synchronize()
        finally:
            hip.lib().td_attention_decode_set_group(prev)
        assert torch.equal(outs[0], outs[1]), f"{what} group {grp}: a repeated launch gave different bits"
        got = outs[0].double().cpu()
        assert torch.isfinite(got).all(), f"{what} group {grp}: a byte or a scale past the end was read"
        r = ((got - ref).abs() / tol).max().item()
        worst = max(worst, r)
        assert r <= 1.0, f"{what} group {grp}: max error {r:.3g} x the bound"
    print(f"{what}: max error {worst:.3f} x the bound")
    return k8, v8, ks, vs, dq, lens, ref, tol


@pytest.mark.parametrize("Hq,Hkv,Skv,B,dom,vmode,uncovered", K.DECODE8_CASES)
def test_decode_attention_kv8_against_float64(hip, Hq, Hkv, Skv, B, dom, vmode, uncovered):
    """|err| <= one bf16 ulp of the float64 reference over the dequantised cache + 2^-12 max |v^| of the kv head, for every forced q-head group that divides
    Hq / Hkv and the automatic choice; a second launch gives identical bits."""
    case = K.decode8_problem(Hq, Hkv, Skv, B, dom, vmode)
    k8, v8, ks, vs, dq, _, ref, tol = _run_decode8(hip, case, uncovered, f"kv8 decode {(Hq, Hkv, Skv, B, dom, vmode)}", use_lens=False)
    if Skv == 17:      # the torch op, and kv_lens naming the full length
        o = _ops().attention_decode_kv8(dq, k8, v8, ks, vs, torch.full((B,), Skv, dtype=torch.int32, device="cuda"), Hq, Hkv, 128 ** -0.5)
        torch.cuda.synchronize()
        assert bool(((o.double().cpu() - ref).abs() <= tol).all())


def test_decode_attention_kv8_unequal_lengths(hip):
    """kv_lens with a different length per sequence, the slot boundaries (1, 2, 15 .. 17, 63 .. 65) among them; everything past a sequence's length is NaN
    bytes under 2^40."""
    lens = [1, 2, 15, 16, 17, 33, 63, 64, 65, 40]
    case = K.decode8_problem(12, 2, 65, len(lens), None, "randn", lens=lens)
    _run_decode8(hip, case, (), "kv8 decode, unequal lengths", use_lens=True)


# ---- 3. the engine ----------------------------------------------------------------------------------------------------------------------------
N0, SLOTS, BATCHES = 40, 66, (1, 3, 17, 64, 65)
LINEAR_KEYS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "gate_proj.weight", "up_proj.weight", "down_proj.weight")


def _tc(cfg):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig
    return Qwen2VLTextConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads, num_key_value_heads=cfg.num_kv_heads,
                             intermediate_size=cfg.intermediate, vocab_size=cfg.vocab, tie_word_embeddings=cfg.tie_embeddings)


def _engine(cfg, sd, max_len, kv="fp8", **kw):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextEngine
    e = Qwen2VLTextEngine(_tc(cfg), max_model_len=max_len, kv_cache_dtype=kv, **kw)
    e.load_state_dict(sd)
    return e


@functools.lru_cache(maxsize=None)
def _problem(w8):
    """Weights, ids and the two references (the restatement with kv_round = the format, in bf16 and in fp32), computed once: the prompt's hidden states, the
    next-token hidden states of 65 sequences that share the prompt, their logits, and two continuations of the prompt.  w8: the oracle runs on W^."""
    cfg = Q.tiny_config()
    sd = Q.init_weights(cfg, seed=31)
    sd_o = {k: (W.quantize_rows(v)[2].to(v.dtype) if (k.endswith(LINEAR_KEYS) or k == "lm_head.weight") else v) for k, v in sd.items()} if w8 else sd
    sd32 = {k: v.float() for k, v in sd_o.items()}
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, cfg.vocab, (N0,), generator=g).to(torch.int32)
    toks = torch.randperm(cfg.vocab, generator=g)[:SLOTS].to(torch.int32)
    cont = torch.randint(0, cfg.vocab, (5,), generator=g).to(torch.int32)
    pos = Q.text_position_ids(N0)
    p16, kv16 = K.text_model_hidden(sd_o, cfg, pos, token_ids=prompt.long(), kv_round=K.kv_round)
    p32, kv32 = K.text_model_hidden(sd32, cfg, pos, token_ids=prompt.long(), kv_round=K.kv_round)
    pos1 = Q.text_position_ids(1, start=N0)
    ref16, ref32, lref = [], [], []
    for b in range(max(BATCHES)):
        h16, _ = K.text_model_hidden(sd_o, cfg, pos1, token_ids=toks[b:b + 1].long(), past=kv16, kv_round=K.kv_round)
        h32, _ = K.text_model_hidden(sd32, cfg, pos1, token_ids=toks[b:b + 1].long(), past=kv32, kv_round=K.kv_round)
        ref16.append(h16[-1])
        ref32.append(h32[-1])
        lref.append(Q.lm_logits(sd_o, cfg, h16[-1]))
    conts = {}
    for n in (1, 5):
        c16, _ = K.text_model_hidden(sd_o, cfg, Q.text_position_ids(n, start=N0), token_ids=cont[:n].long(), past=kv16, kv_round=K.kv_round)
        c32, _ = K.text_model_hidden(sd32, cfg, Q.text_position_ids(n, start=N0), token_ids=cont[:n].long(), past=kv32, kv_round=K.kv_round)
        conts[n] = (c16, c32)
    return dict(cfg=cfg, sd=sd, prompt=prompt, toks=toks, cont=cont, pos=pos, p16=p16, p32=p32, ref16=torch.stack(ref16), ref32=torch.stack(ref32),
                lref=torch.stack(lref), conts=conts)


def _prefill(hip, e, entry, prompt, pos, slot=0):
    """The prompt into `slot` through one of the three prefill entries -> its hidden states [n, D]."""
    n = prompt.numel()
    if entry == "forward":
        return e.forward(pos, prompt, slot=slot)[0]
    tok, p = prompt.cuda(), pos.to(torch.int32).cuda().contiguous()
    hid = torch.empty(n, e.config.hidden_size, dtype=torch.bfloat16, device="cuda")
    lens = (ctypes.c_int * 1)(n)
    if entry == "batch":
        hip.check(e._L.td_qwen2_prefill_batch_at(e._h, slot, 1, n, hip.ptr(tok), None, hip.ptr(p), ctypes.cast(lens, ctypes.c_void_p), hip.ptr(hid), None, hip.stream_ptr()))
    else:
        hip.check(e._L.td_qwen2_prefill_packed(e._h, slot, 1, hip.ptr(tok), None, hip.ptr(p), ctypes.cast(lens, ctypes.c_void_p), hip.ptr(hid), None, hip.stream_ptr()))
    torch.cuda.synchronize()
    return hid


def _assert_fixed_points(rows, what):
    """Every head vector re-quantises to itself, and its amax 2^-e lies in (224, 448] -- or it is zero."""
    r = rows.float().cpu()
    heads = r.shape[1] // 128
    q, scale, hat, e = K.quantize_kv_rows(r, heads)
    assert torch.equal(hat, r), f"{what}: a cache row is not a fixed point of the format"
    am = r.reshape(-1, 128).abs().amax(dim=1).double() * torch.exp2(-e.reshape(-1).double())
    assert bool(((am == 0) | ((am > 224.0) & (am <= 448.0))).all()), what


@pytest.mark.parametrize("entry,w8", [("forward", False), ("batch", False), ("packed", False), ("forward", True)])
def test_engine_decode_with_e4m3_cache(hip, entry, w8):
    P = _problem(w8)
    cfg, prompt, toks, pos = P["cfg"], P["prompt"], P["toks"], P["pos"]
    Hkv, KVW = cfg.num_kv_heads, 2 * cfg.num_kv_heads * 128
    e = _engine(cfg, P["sd"], max_len=SLOTS * 128)
    ref_bytes = cfg.num_layers * SLOTS * 128 * (KVW + 8 * Hkv)
    assert e.kv_cache_info() == {"dtype": "fp8", "bytes_per_row": KVW + 8 * Hkv, "cache_bytes": ref_bytes}
    if entry == "forward" and not w8:
        e16 = _engine(cfg, P["sd"], max_len=SLOTS * 128, kv="auto")
        i16 = e16.kv_cache_info()
        assert i16 == {"dtype": "auto", "bytes_per_row": 2 * KVW, "cache_bytes": cfg.num_layers * SLOTS * 128 * 2 * KVW}
        assert ref_bytes * 2 * KVW == i16["cache_bytes"] * (KVW + 8 * Hkv) and abs(ref_bytes / i16["cache_bytes"] - 0.516) < 5e-4
        del e16

    def prepare(eng):
        """The prompt into slot 0 through the entry under test, then copied to every other slot."""
        if w8:
            eng.quantize_weights("fp8")
        eng.set_slots(SLOTS)
        assert eng.slot_len == 128
        hid = _prefill(hip, eng, entry, prompt, pos)
        for b in range(1, SLOTS):
            eng.move_slot(0, b, N0)
        return hid

    hid_p = prepare(e)
    ep = _rel(P["p16"], P["p32"])
    print(f"{entry} w8={w8} prefill: rel-RMSE hip~bf16 {_rel(hid_p, P['p16']):.4f} hip~fp32 {_rel(hid_p, P['p32']):.4f} bf16~fp32 {ep:.4f}")
    assert _rel(hid_p, P["p16"]) < 2e-2 and _rel(hid_p, P["p32"]) < 1.5 * ep + 2e-3
    for layer in range(cfg.num_layers):
        _assert_fixed_points(e.read_kv(layer, 0, 0, N0), f"{entry} prefill layer {layer}")
    assert torch.equal(e.read_kv(1, SLOTS - 1, 0, N0), e.read_kv(1, 0, 0, N0))          # both planes moved
    # The separate rope / cache-write launch gets a handle of its own, in that form from its first step: on one handle it would find the rows the fused
    # form had left and could store nothing, or store elsewhere, unseen.
    e_sep = None
    if entry == "forward":
        e_sep = _engine(cfg, P["sd"], max_len=SLOTS * 128)
        assert torch.equal(prepare(e_sep), hid_p)
        assert e_sep.set_fused_rope(False) is True

    def blank_new_rows(eng, B):
        """Row N0 of slots 0 .. B-1 back to the zeros of creation (bytes and scales): the last slot is never stepped, so its rows [0, N0] are the prompt and
        one untouched row.  What a step leaves in row N0 is then what THAT step stored."""
        for b in range(B):
            eng.move_slot(SLOTS - 1, b, N0 + 1)
        for layer in range(cfg.num_layers):
            assert not eng.read_kv(layer, B - 1, N0, 1).any() and not eng.read_kv(layer, 0, N0, 1).any()

    def new_rows(eng, B):
        return [torch.cat([eng.read_kv(layer, b, N0, 1) for b in range(B)]) for layer in range(cfg.num_layers)]      # row N0 of EVERY stepped slot

    def step(eng, B, slots=None):
        """Eager, captured, replayed -> hidden states, logits, and the new cache rows as the FIRST (eager) call left them in blank rows."""
        blank_new_rows(eng, B)
        first = eng.decode_batch(toks[:B], torch.full((3, B), N0, dtype=torch.int32), [N0] * B, slots=slots)
        rows = new_rows(eng, B)
        outs = [first] + [eng.decode_batch(toks[:B], torch.full((3, B), N0, dtype=torch.int32), [N0] * B, slots=slots) for _ in range(2)]
        torch.cuda.synchronize()
        for h, lg in outs[1:]:
            assert torch.equal(h, outs[0][0]) and torch.equal(lg, outs[0][1]), f"B={B}: eager, captured and replayed steps differ"
        for a, b in zip(rows, new_rows(eng, B)):
            assert torch.equal(a, b), f"B={B}: the captured / replayed steps left other cache rows than the eager one"
        return outs[0][0].clone(), outs[0][1].clone(), rows

    assert max(BATCHES) < SLOTS
    for B in BATCHES:
        h, lg, new = step(e, B)
        eref = _rel(P["ref16"][:B], P["ref32"][:B])
        e16, e32 = _rel(h, P["ref16"][:B]), _rel(h, P["ref32"][:B])
        print(f"{entry} w8={w8} B={B}: rel-RMSE hip~bf16 {e16:.4f} hip~fp32 {e32:.4f} bf16~fp32 {eref:.4f} logits {_rel(lg, P['lref'][:B]):.4f}")
        assert e16 < 2e-2 and e32 < 1.5 * eref + 2e-3
        assert _rel(lg, P["lref"][:B]) < 3e-2
        for layer, r in enumerate(new):
            assert r.shape[0] == B and bool(r.any(dim=1).all()), f"B={B} layer {layer}: a stepped slot's new row was not written"
            _assert_fixed_points(r, f"B={B} new rows, layer {layer}")
        if e_sep is not None:
            # the same hidden states, logits and new cache rows (every stepped slot), bit for bit, from the handle that only ever ran the separate launch
            h2, lg2, new2 = step(e_sep, B)
            assert torch.equal(h, h2) and torch.equal(lg, lg2), f"B={B}: fused and separate rope differ"
            for layer, (a, b) in enumerate(zip(new, new2)):
                assert torch.equal(a, b), f"B={B} layer {layer}: the new cache rows differ between the fused and the separate rope"
            # a step from moved slots equals the step from their source: rows of the result permute with the slots
            if B > 1:
                perm = list(range(B - 1, -1, -1))
                hp, lp, newp = step(e, B, slots=perm)
                assert torch.equal(hp, h) and torch.equal(lp, lg), f"B={B}: a step from moved slots differs from its source's"
                for a, b in zip(new, newp):
                    assert torch.equal(a, b.flip(0)), f"B={B}: sequence b's new row did not land in the slot it named"


@pytest.mark.parametrize("n", [1, 5])
def test_forward_continuation_reads_the_staged_cache(hip, n):
    """forward(pos0 = 40, n) on an 8-bit handle: the slot's rows are dequantised into the staging rows, the new rows join them, the bf16 attention runs."""
    P = _problem(False)
    cfg = P["cfg"]
    e = _engine(cfg, P["sd"], max_len=128)
    e.forward(P["pos"], P["prompt"])
    h, _ = e.forward(Q.text_position_ids(n, start=N0), P["cont"][:n], pos0=N0)
    torch.cuda.synchronize()
    c16, c32 = P["conts"][n]
    eref = _rel(c16, c32)
    print(f"continuation n={n}: rel-RMSE hip~bf16 {_rel(h, c16):.4f} hip~fp32 {_rel(h, c32):.4f} bf16~fp32 {eref:.4f}")
    assert _rel(h, c16) < 2e-2 and _rel(h, c32) < 1.5 * eref + 2e-3
    for layer in range(cfg.num_layers):
        _assert_fixed_points(e.read_kv(layer, 0, 0, N0 + n), f"continuation layer {layer}")
    if n == 1:      # one token through the staging path against the same token through the decode step (the reference's bars between them)
        e2 = _engine(cfg, P["sd"], max_len=128)
        e2.forward(P["pos"], P["prompt"])
        hd, _ = e2.decode_batch(P["cont"][:1], torch.full((3, 1), N0, dtype=torch.int32), [N0])
        torch.cuda.synchronize()
        assert _rel(hd, c16) < 2e-2 and _rel(hd, h) < 2e-2
        for layer in range(cfg.num_layers):
            assert _rel(e2.read_kv(layer, 0, N0, 1), e.read_kv(layer, 0, N0, 1)) < 2e-2


def test_bf16_mode_through_create_kv_is_create_ex(hip):
    """td_qwen2_create_kv(..., TD_QWEN2_KV_BF16) and td_qwen2_create_ex give the same bits for prefill + decode (and the same cache rows)."""
    P = _problem(False)
    cfg = P["cfg"]

    def run(via_ex):
        e = _engine(cfg, P["sd"], max_len=4 * 128, kv="auto")
        if via_ex:      # the same engine object on a handle made by the older entry
            cc = hip.TdQwen2Config(cfg.hidden, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, 128, cfg.intermediate, cfg.vocab, 0, (ctypes.c_int * 3)(16, 24, 24),
                                   cfg.rms_eps, cfg.rope_theta)
            h = ctypes.c_void_p()
            hip.check(e._L.td_qwen2_create_ex(ctypes.byref(cc), 4 * 128, 1, 4 * 128, ctypes.byref(h)))
            e._L.td_qwen2_destroy(e._h)
            e._h = h
            e.load_state_dict(P["sd"])
        assert e.kv_cache_info()["dtype"] == "auto"
        e.set_slots(4)
        hp, _ = e.forward(P["pos"], P["prompt"])
        for b in (1, 2):
            e.move_slot(0, b, N0)
        hd, lg = e.decode_batch(P["toks"][:3], torch.full((3, 3), N0, dtype=torch.int32), [N0] * 3)
        kv = e.read_kv(1, 2, 0, N0 + 1)
        torch.cuda.synchronize()
        return hp.clone(), hd.clone(), lg.clone(), kv.clone()

    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)


# ---- 4. get_embed -----------------------------------------------------------------------------------------------------------------------------
def test_get_embed_with_fp8_kv_cache(hip):
    """ThinkDiff-LVLM get_embed, teacher-forced as tests/test_qwen2_w8_gpu.py::test_get_embed_with_fp8_quantization, with vllm_config["kv_cache_dtype"] =
    "fp8": the aligner restatement on the rounding oracle, within that test's 3e-2; without the key the model is bit-equal to one built as before."""
    from oracle import aligner_ref as A
    from thinkdiff.models.mllama_vllm_t5_embed_decoder_2 import MllamaVllmT5EmbedDecoderForConditionalGeneration_5
    cfg = Q.tiny_config()
    sd = Q.init_weights(cfg, seed=9)
    asd = A.init_weights(cfg.hidden, 4096, seed=4)
    tc = _tc(cfg)
    base = {"max_model_len": 256, "max_tokens": 6, "min_tokens": 6}
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, cfg.vocab, (20,), generator=g).tolist()
    forced = torch.randint(0, cfg.vocab, (6,), generator=g).tolist()

    def build(vc):
        m = MllamaVllmT5EmbedDecoderForConditionalGeneration_5(tc, vllm_config=vc)
        m.mllama.load_state_dict(sd)
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

    for name in ("fp8", "fp8_e4m3"):
        m8 = build({**base, "kv_cache_dtype": name})
        assert m8.mllama.kv_cache_info()["dtype"] == "fp8" and m8.mllama.weight_info()["mode"] == "bf16"
        ref_h, _ = K.text_model_hidden(sd, cfg, Q.text_position_ids(26), token_ids=torch.tensor(prompt + forced), kv_round=K.kv_round)
        for et, sl in [("both", slice(0, 26)), ("output_embed", slice(20, 26))]:
            got = run(m8, et)
            assert got.shape == (sl.stop - sl.start, 4096)
            assert _rel(got, ref_aligner(ref_h[sl])) < 3e-2
        del m8
    # no key, "auto" or None: today's model, bit for bit -- a bf16 cache, and the bits of a handle made by td_qwen2_create_ex (tested above)
    a, b, c = run(build(dict(base))), run(build({**base, "kv_cache_dtype": "auto"})), run(build({**base, "kv_cache_dtype": None}))
    assert torch.equal(a, b) and torch.equal(a, c)
    ref_plain, _ = Q.text_model_hidden(sd, cfg, Q.text_position_ids(26), token_ids=torch.tensor(prompt + forced))
    assert _rel(a, ref_aligner(ref_plain)) < 3e-2
    plain = MllamaVllmT5EmbedDecoderForConditionalGeneration_5(tc, vllm_config=dict(base))
    assert plain.mllama.kv_cache_dtype == "auto" and plain.mllama.kv_cache_info()["dtype"] == "auto"
