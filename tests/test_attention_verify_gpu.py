"""Multi-row decode attention (td_attention_verify) and the accept rule of speculative decoding (td_spec_accept) on the GPU.

T1: row (b, j) of td_attention_verify against the single-row decode kernel on one query with len0[b] + j keys of the same cache-shaped buffer --
hip.attention (Sq = 1, causal, k[:, :len0 + j]) for the bf16 cache, attention_decode_kv8 with kv_lens for the e4m3 cache -- in both forms (one
workgroup per row, the multi-row kernel), under every q-head group that divides Hq / Hkv and the automatic choice (the partner runs under the same
setting), twice.
  form 1 (one workgroup per row: the single-row kernel's own body): the BITS of the partner, torch.equal.
  form 2 (the multi-row kernel): equality with the partner was NOT reached.  The compiler contracts the single-row kernel's softmax update into
  fmas differently from one of its key loops to the next; the multi-row kernel writes one contraction out, and a fraction of a per cent of the rows
  then differ from the partner in the last bf16 bit (measured on the MI355X: 0 - 10 of up to 266 rows per case).  So form 2 is held
  to the float64 bound of tests/test_attention_gpu.py::test_decode_against_cache -- one bf16 ulp of the reference plus 2^-12 max |v| of the kv head
  -- and, because its arithmetic is written out, to giving the SAME bits under every group and row chunk.
T2: td_spec_accept against a numpy loop, exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T_SET = (1, 2, 3, 5, 8)
SMALL = (1, 2, 15, 16, 17, 63, 64, 65, 129)
HEADS = [(12, 2), (28, 4), (4, 4), (7, 1)]
# len0 of every sequence: all of {1, 2, 15, 16, 17, 63, 64, 65, 129, 300, 1025} occur, the long ones where few sequences keep the buffers small
LEN0 = {
    1: {(12, 2): [1], (28, 4): [2], (4, 4): [16], (7, 1): [64]},
    3: {(12, 2): [300, 1025, 15], (28, 4): [17, 300, 63], (4, 4): [65, 1025, 129], (7, 1): [1025, 2, 300]},
    70: {h: [SMALL[(i + k) % len(SMALL)] for i in range(70)] for k, h in enumerate(HEADS)},
}


def _layout(n_seq, len0, seed):
    """-> t, row0 (with gaps: q / o rows no sequence owns), slots (permuted, non-contiguous), n_slots, R (rows of q / o), S (rows of a slot)."""
    rng = np.random.default_rng(seed)
    t = np.array([T_SET[(i + seed) % len(T_SET)] for i in range(n_seq)], dtype=np.int32)
    if n_seq >= 5:
        assert set(t.tolist()) == set(T_SET)
    gaps = np.array([i % 2 for i in range(n_seq)], dtype=np.int32)
    row0 = (np.concatenate([[0], np.cumsum(t + gaps)[:-1]]) + 1).astype(np.int32)
    n_slots = n_seq + 3
    slots = rng.permutation(n_slots)[:n_seq].astype(np.int32)
    R = int(row0[-1] + t[-1] + 1)
    S = int(max(l + k for l, k in zip(len0, t)) - 1 + 7)
    return t, row0, slots, n_slots, R, S


def _cache_bf16(n_slots, S, Hkv, slots, len0, t, gen):
    """[n_slots, S, ld] bf16 on the device, k | v | pad columns; every row no query may see -- past len0 + t - 1 of a used slot, all of an unused
    one -- is 1e4, which would dominate every score and value if read."""
    ld = 2 * Hkv * 128 + 64
    buf = torch.randn(n_slots, S, ld, generator=gen, device="cuda")
    keep = torch.zeros(n_slots, dtype=torch.int64)
    keep[torch.from_numpy(slots.astype(np.int64))] = torch.from_numpy((np.asarray(len0) + t - 1).astype(np.int64))
    past = torch.arange(S, device="cuda")[None, :] >= keep.cuda()[:, None]
    buf[past] = 1e4
    return buf.bfloat16()


def _partner_bf16(hip, q, cache, Hq, Hkv, row_of, slot_of, len_of):
    """The single-row kernel, one launch per distinct length: the rows of that length against copies of their slots' first `length` rows."""
    out = {}
    by_len = {}
    for r, s, n in zip(row_of, slot_of, len_of):
        by_len.setdefault(int(n), []).append((int(r), int(s)))
    for n, rs in by_len.items():
        rows = torch.tensor([r for r, _ in rs], device="cuda")
        sl = torch.tensor([s for _, s in rs], device="cuda")
        kv = cache.index_select(0, sl)[:, :n]
        qq = q.index_select(0, rows)[:, None, :]
        o = torch.empty(len(rs), 1, Hq * 128, dtype=torch.bfloat16, device="cuda")
        hip.attention(qq, kv[:, :, :Hkv * 128], kv[:, :, Hkv * 128:2 * Hkv * 128], o, Hq, Hkv, causal=True)
        for i, (r, _) in enumerate(rs):
            out[r] = o[i, 0]
    return out


def _ref64(q, values, Hq, Hkv, n_seq, t, row0, slots, len0):
    """float64 attention of every owned row on `values` [n_slots, S, >= 2 Hkv 128] (what the cache holds, exactly) -> {q row: (ref [Hq 128], bound)};
    bound = one bf16 ulp of the reference + 2^-12 max |v| over the row's visible keys of its kv head."""
    out, rep = {}, Hq // Hkv
    for b in range(n_seq):
        L = int(len0[b]) + int(t[b]) - 1
        kv = values[int(slots[b]), :L].double()
        k, v = kv[:, :Hkv * 128].reshape(L, Hkv, 128), kv[:, Hkv * 128:2 * Hkv * 128].reshape(L, Hkv, 128)
        qq = q[int(row0[b]):int(row0[b]) + int(t[b])].double().reshape(int(t[b]), Hkv, rep, 128)
        sc = torch.einsum("thrd,lhd->thrl", qq, k) * 128 ** -0.5
        seen = torch.arange(L, device=q.device)[None, :] < (int(len0[b]) + torch.arange(int(t[b]), device=q.device))[:, None]      # [t, L]
        sc = sc.masked_fill(~seen[:, None, None, :], float("-inf"))
        ref = torch.einsum("thrl,lhd->thrd", torch.softmax(sc, dim=-1), v).reshape(int(t[b]), Hq * 128)
        vmax = torch.cummax(v.abs().amax(dim=2), dim=0).values      # [L, Hkv]: over keys 0 .. l
        for j in range(int(t[b])):
            vm = vmax[int(len0[b]) + j - 1].repeat_interleave(rep * 128)
            tol = torch.exp2(torch.floor(torch.log2(ref[j].abs().clamp_min(2.0 ** -126))) - 7) + 2.0 ** -12 * vm
            out[int(row0[b]) + j] = (ref[j], tol)
    return out


def _run(hip, Hq, Hkv, n_seq, len0, kv8, seed):
    t, row0, slots, n_slots, R, S = _layout(n_seq, len0, seed)
    gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
    cache = _cache_bf16(n_slots, S, Hkv, slots, len0, t, gen)
    ld = cache.shape[2]
    qbuf = torch.randn(R, Hq * 128 + 64, generator=gen, device="cuda").bfloat16()
    q = qbuf[:, :Hq * 128]
    row_of = [int(row0[b]) + j for b in range(n_seq) for j in range(t[b])]
    slot_of = [int(slots[b]) for b in range(n_seq) for j in range(t[b])]
    len_of = [int(len0[b]) + j for b in range(n_seq) for j in range(t[b])]
    if kv8:
        flat = cache.reshape(n_slots * S, ld)
        safe = torch.where(flat[:, :2 * Hkv * 128].float().abs() > 100, torch.zeros((), device="cuda"), flat[:, :2 * Hkv * 128].float()).bfloat16()
        by, sc, hat = hip.kv_quant_rows_e4m3(safe.contiguous(), 2 * Hkv)
        values = hat.reshape(n_slots, S, 2 * Hkv * 128)      # x^: what the bytes and scales hold, exactly
        # planes with pad columns; what must not be read: byte 0x7F (e4m3 NaN), scale 2^40
        qb = torch.full((n_slots * S, 2 * Hkv * 128 + 64), 0x7F, dtype=torch.uint8, device="cuda")
        sb = torch.full((n_slots * S, 2 * Hkv + 3), 2.0 ** 40, dtype=torch.float32, device="cuda")
        seen = (flat[:, 0].float() < 100)
        qb[seen, :2 * Hkv * 128] = by[seen]
        sb[seen, :2 * Hkv] = sc[seen]
        qb, sb = qb.reshape(n_slots, S, -1), sb.reshape(n_slots, S, -1)
        cache_arg = (qb[:, :, :Hkv * 128], qb[:, :, Hkv * 128:2 * Hkv * 128], sb[:, :, :Hkv], sb[:, :, Hkv:2 * Hkv])
        sl = torch.tensor(slot_of, device="cuda")
        ex = [p.index_select(0, sl) for p in cache_arg]
        q_rows, lens_dev = q.index_select(0, torch.tensor(row_of, device="cuda")), torch.tensor(len_of, dtype=torch.int32, device="cuda")

        def partner():
            return hip.attention_decode_kv8(q_rows, *ex, Hq, Hkv, kv_lens=lens_dev)
    else:
        cache_arg = (cache[:, :, :Hkv * 128], cache[:, :, Hkv * 128:2 * Hkv * 128])
        values = cache

        def partner():
            got = _partner_bf16(hip, q, cache, Hq, Hkv, row_of, slot_of, len_of)
            return torch.stack([got[r] for r in row_of])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    d_row0, d_t, d_len0, d_slot = dev(row0), dev(t), dev(np.asarray(len0)), dev(slots)
    rows_idx = torch.tensor(row_of, device="cuda")
    owned = torch.zeros(R, dtype=torch.bool, device="cuda")
    owned[rows_idx] = True
    L = hip.lib()
    r64 = _ref64(q, values, Hq, Hkv, n_seq, t, row0, slots, len0)
    ref, tol = torch.stack([r64[r][0] for r in row_of]), torch.stack([r64[r][1] for r in row_of])
    form2, worst, differ = None, 0.0, 0
    for form in (1, 2):
        for grp in [0] + [g for g in (1, 2, 3, 4, 6, 7) if (Hq // Hkv) % g == 0]:
            pf, pg = L.td_attention_verify_set_form(form), L.td_attention_decode_set_group(grp)
            try:
                want = partner()      # the single-row kernel under the same forced group
                assert torch.isfinite(want.float()).all()
                outs = []
                for _ in range(2):
                    obuf = torch.full((R, Hq * 128 + 64), -7.0, dtype=torch.bfloat16, device="cuda")
                    hip.attention_verify(q, cache_arg, d_row0, d_t, d_len0, d_slot, Hq, Hkv, out=obuf[:, :Hq * 128])
                    outs.append(obuf)
                torch.cuda.synchronize()
            finally:
                L.td_attention_verify_set_form(pf)
                L.td_attention_decode_set_group(pg)
            what = f"form {form} group {grp} (Hq {Hq}, Hkv {Hkv}, {n_seq} sequences, kv8 {kv8})"
            assert torch.equal(outs[0], outs[1]), f"{what}: a repeated launch gave different bits"
            got = outs[0][:, :Hq * 128].index_select(0, rows_idx)
            assert torch.isfinite(got.float()).all(), f"{what}: a row past a sequence's end was read"
            bad = (got != want).any(dim=1).nonzero().flatten().tolist()
            if form == 1:
                assert not bad, f"{what}: rows {[(row_of[i], len_of[i]) for i in bad[:8]]} (q row, keys) differ from the single-row kernel"
            else:
                differ = max(differ, len(bad))
                r = ((got.double() - ref).abs() / tol).max().item()
                worst = max(worst, r)
                assert r <= 1.0, f"{what}: max error {r:.3g} x the float64 bound"
                if form2 is None:
                    form2 = got
                assert torch.equal(got, form2), f"{what}: the multi-row kernel gave other bits than under the automatic group"
            assert (outs[0][~owned] == -7.0).all() and (outs[0][:, Hq * 128:] == -7.0).all(), f"{what}: a row or column nobody owns was written"
    print(f"Hq {Hq} Hkv {Hkv} n_seq {n_seq} kv8 {kv8}: form 2 max error {worst:.3f} x the float64 bound, up to {differ} of {len(row_of)} rows differ from the single-row kernel")


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("n_seq", [1, 3, 70])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_verify_rows_equal_single_row_kernel(hip, Hq, Hkv, n_seq, kv8):
    _run(hip, Hq, Hkv, n_seq, LEN0[n_seq][(Hq, Hkv)], kv8, seed=HEADS.index((Hq, Hkv)) + 3 * n_seq)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "e4m3"])
def test_verify_rows_long_cache(hip, kv8):
    """One sequence of 8192 keys with 8 rows."""
    Hq, Hkv = (28, 4) if kv8 else (12, 2)
    _run(hip, Hq, Hkv, 1, [8192], kv8, seed=4)      # seed 4 -> t = T_SET[4] = 8


def _accept_ref(sampled, fed, row0, t):
    B = len(row0)
    n_emit, emit = np.zeros(B, dtype=np.int32), np.full((B, 8), -1, dtype=np.int32)
    for b in range(B):
        a = 0
        while a < t[b] - 1 and fed[row0[b] + a + 1] == sampled[row0[b] + a]:
            a += 1
        n_emit[b] = a + 1
        emit[b, :a + 1] = sampled[row0[b]:row0[b] + a + 1]
    return n_emit, emit


@pytest.mark.parametrize("B", [1, 3, 256])
def test_spec_accept_against_numpy(hip, B):
    """Per sequence one of: no draft (t = 1), all accepted, the first draft rejected, a rejection in the middle, t = 8 (all accepted and a late
    rejection); rows are laid out back to back with a gap in front."""
    rng = np.random.default_rng(B)
    kinds = ["none", "all", "first", "middle", "all8", "late8"]
    t, fed_l, smp_l = [], [], []
    for b in range(B):
        kind = kinds[(b + B) % len(kinds)] if B > 1 else "middle"
        tb = {"none": 1, "all": 4, "first": 3, "middle": 5, "all8": 8, "late8": 8}[kind]
        fed = rng.integers(0, 1000, tb)
        smp = np.concatenate([fed[1:], rng.integers(0, 1000, 1)])      # every draft right ...
        wrong = {"first": 0, "middle": 2, "late8": 6}.get(kind)
        if wrong is not None:
            smp[wrong] = fed[wrong + 1] + 1                             # ... but this one
        t.append(tb); fed_l.append(fed); smp_l.append(smp)
    t = np.array(t, dtype=np.int32)
    row0 = (np.concatenate([[0], np.cumsum(t)[:-1]]) + 2).astype(np.int32)
    fed = np.concatenate([[7, 7]] + fed_l).astype(np.int32)
    smp = np.concatenate([[9, 9]] + smp_l).astype(np.int32)
    want_n, want_e = _accept_ref(smp, fed, row0, t)
    if B > 3:
        assert {1, 3, 4, 7, 8} <= set(want_n.tolist())
    n_emit, emit = hip.spec_accept(torch.from_numpy(smp).cuda(), torch.from_numpy(fed).cuda(), torch.from_numpy(row0).cuda(), torch.from_numpy(t).cuda())
    assert np.array_equal(n_emit.cpu().numpy(), want_n)
    assert np.array_equal(emit.cpu().numpy(), want_e)
