"""Operands, float64 references and reference mutants of the packed causal and cached-prefill attention cases, shared by
tests/test_attention_cases_cpu.py (which asserts that every mutant lies >= 10x the GPU test's bar from the reference) and
tests/test_attention_packed_gpu.py (which runs the kernels on the same operands).  CPU torch only.

The bar of both GPU tests is the one of tests/test_attention_gpu.py: |err| <= 2^-7 max|ref|, the maximum taken per segment (packed) or
per batch entry (cached prefill).  Random operands alone do not make that bar decisive: a mask that is one key off moves an average over
hundreds of keys by less than the bar.  So keys are PLANTED.  For a query row r and the kv head of a q-head group,
    k[x] = 3 * sum_{h in group} q[r, h]
makes key x the dominant one of row r for every head of the group (q_h . k[x] * scale ~ 3 * 128 * 128^-0.5 ~ 34 against scores of
standard deviation 1).  x = r + 1 (a SUCCESSOR plant): the first key beyond the diagonal would take the row over if the kernel saw it.
x = r (a DIAGONAL plant): the row is its own value row, and losing the diagonal key changes it completely.
"""
import math

import torch

D = 128
SCALE = D ** -0.5
BAR = 2.0 ** -7
MIN_MARGIN = 10.0

# ---- packed causal segments (td_attention_segments_bf16, causal = 1) ---------------------------------------------------------------------------------

# the wave's 32 rows, the 64-key tile, the 256-row workgroup, a second query tile with a ragged end; one-row segments first and last
PACKED_LENS = [1, 2, 31, 32, 33, 64, 65, 255, 256, 257, 300, 513, 1]
PACKED_HEADS = [(4, 2), (7, 1)]
# Offsets (inside a segment) asked for each plant kind.  A successor plant at row r and a diagonal plant at row r + 1 would both own key r + 1, and
# a row cannot carry both kinds, so ONE SEGMENT cannot hold both kinds at all of 31, 32, 63, 64, 255, 256.  Segments therefore alternate between two
# layouts: layout 0 has the successor plants at the six offsets (diagonal plants one row in front of each pair), layout 1 the diagonal plants
# (successor plants one row behind each pair).  Segment s of a launch takes layout (s + flip) % 2, flip = 0 for the first head configuration and 1
# for the second; several segments are long enough for every offset, so EVERY launch carries both kinds at all six offsets
# (tests/test_attention_cases_cpu.py asserts it), each kind in segments of different lengths in the two launches.  The last row of every segment is
# a successor row (its key is the NEXT segment's first row, or the spare row behind the last segment), the row before it a diagonal row.
PACKED_EDGES = [31, 32, 63, 64, 255, 256]
PACKED_LAYOUTS = [{"succ": PACKED_EDGES, "diag": [30, 62, 254]}, {"succ": [33, 65, 257], "diag": PACKED_EDGES}]
PAD = 1.0e4        # pad columns of the operand rows: finite, so that the float64 side can hold the same buffer, and fatal to any score or value read from them


def packed_plants(Hq, Hkv):
    """[(succ rows, diag rows)] per segment, as offsets inside the segment: disjoint, no key owned twice, row 0 never a diagonal row (it
    has no 'one key fewer')."""
    flip = PACKED_HEADS.index((Hq, Hkv))
    out = []
    for s, n in enumerate(PACKED_LENS):
        want = PACKED_LAYOUTS[(s + flip) % 2]
        succ, diag = [n - 1], ([n - 2] if n - 2 >= 1 else [])
        keys = {n} | set(diag)                                  # keys already owned (segment-local index; n = the next segment's first row)
        for r in want["succ"]:
            if r < n - 1 and r not in succ and r not in diag and r + 1 not in keys:
                succ.append(r)
                keys.add(r + 1)
        for r in want["diag"]:
            if 1 <= r < n - 1 and r not in succ and r not in diag and r not in keys:
                diag.append(r)
                keys.add(r)
        out.append((sorted(succ), sorted(diag)))
    return out


def _group_sum(qrow, Hq, Hkv):
    """q row [Hq*128] -> 3 * sum over each kv head's q heads, [Hkv*128] (float32)."""
    return 3.0 * qrow.float().reshape(Hkv, Hq // Hkv, D).sum(dim=1).reshape(Hkv * D)


_packed = {}


def packed_case(Hq, Hkv):
    """One launch's operands: dict with
    buf     bf16 [S + 1, ld]: q | 8 pad | k | 8 pad | v | 40 pad columns per row (pad columns hold PAD); row S is a spare row behind the last segment
            (it holds the successor plant of the last row and belongs to no segment)
    q, k, v views of buf's first S rows (columns q0, k0, v0), starts (int32 [n_seg + 1]), lens, plants, S, ld, cols
    ref     float64 [S, Hq*128]: causal attention inside each segment
    Built once per head configuration and never modified."""
    key = (Hq, Hkv)
    if key in _packed:
        return _packed[key]
    g = torch.Generator().manual_seed(1000 * Hq + Hkv)
    lens = PACKED_LENS
    S = sum(lens)
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    QW, KW = Hq * D, Hkv * D
    q0, k0 = 0, QW + 8
    v0 = k0 + KW + 8
    ld = v0 + KW + 40
    buf = torch.randn(S + 1, ld, generator=g)
    plants = packed_plants(Hq, Hkv)
    qb = buf[:, q0:q0 + QW].bfloat16()                       # the plants are built from q as the kernel reads it
    for s, (succ, diag) in enumerate(plants):
        r0 = starts[s]
        for r in succ:
            buf[r0 + r + 1, k0:k0 + KW] = _group_sum(qb[r0 + r], Hq, Hkv)
        for r in diag:
            buf[r0 + r, k0:k0 + KW] = _group_sum(qb[r0 + r], Hq, Hkv)
    for a, b in ((QW, k0), (k0 + KW, v0), (v0 + KW, ld)):
        buf[:, a:b] = PAD
    buf = buf.bfloat16()
    case = dict(Hq=Hq, Hkv=Hkv, lens=lens, starts=torch.tensor(starts, dtype=torch.int32), S=S, ld=ld, cols=(q0, k0, v0), buf=buf, plants=plants,
                q=buf[:S, q0:q0 + QW], k=buf[:S, k0:k0 + KW], v=buf[:S, v0:v0 + KW])
    case["ref"] = packed_ref(case)
    _packed[key] = case
    return case


def _heads64(case):
    """q [Hq, S + 1, 128], k, v [Hkv, S + 1, 128] in float64 over ALL rows of the buffer (the spare row included)."""
    Hq, Hkv, buf = case["Hq"], case["Hkv"], case["buf"]
    q0, k0, v0 = case["cols"]
    R = buf.shape[0]
    q = buf[:, q0:q0 + Hq * D].double().reshape(R, Hq, D).transpose(0, 1)
    k = buf[:, k0:k0 + Hkv * D].double().reshape(R, Hkv, D).transpose(0, 1)
    v = buf[:, v0:v0 + Hkv * D].double().reshape(R, Hkv, D).transpose(0, 1)
    return q, k, v


def packed_ref(case, causal=True, lead=0, kv_of=None):
    """float64 attention inside each packed segment -> [S, Hq*128].  The mutants of the whole launch are arguments:
    lead = 1: every segment also sees the row in front of its start (the first segment has none); causal = False: full attention
    inside each segment; kv_of: q head -> kv head map (default head // (Hq / Hkv))."""
    Hq, Hkv, S = case["Hq"], case["Hkv"], case["S"]
    q, k, v = _heads64(case)
    kv = [h // (Hq // Hkv) for h in range(Hq)] if kv_of is None else kv_of
    kq, vq = k[kv], v[kv]                                                                      # [Hq, S + 1, 128]
    out = torch.empty(S, Hq * D, dtype=torch.float64)
    starts = case["starts"].tolist()
    for s, n in enumerate(case["lens"]):
        r0 = starts[s]
        a = max(r0 - lead, 0)                                                                   # first key row
        sc = q[:, r0:r0 + n] @ kq[:, a:r0 + n].transpose(1, 2) * SCALE                          # [Hq, n, keys]
        if causal:
            i = torch.arange(n)[:, None] + (r0 - a)
            sc = sc.masked_fill(torch.arange(r0 + n - a)[None, :] > i, float("-inf"))
        o = torch.softmax(sc, dim=-1) @ vq[:, a:r0 + n]
        out[r0:r0 + n] = o.transpose(0, 1).reshape(n, Hq * D)
    return out


def packed_row(case, s, r, n_keys):
    """float64 output row r of segment s when it sees the n_keys rows from the segment's start on (the true row: n_keys = r + 1; the
    key behind a segment's last row is the next segment's first row or the spare row) -> [Hq*128]."""
    Hq, Hkv = case["Hq"], case["Hkv"]
    q, k, v = _heads64(case)
    kv = [h // (Hq // Hkv) for h in range(Hq)]
    r0 = int(case["starts"][s])
    sc = (q[:, r0 + r:r0 + r + 1] @ k[kv][:, r0:r0 + n_keys].transpose(1, 2)) * SCALE
    return (torch.softmax(sc, dim=-1) @ v[kv][:, r0:r0 + n_keys]).reshape(Hq * D)


def segment_margins(case, mutant):
    """max |mutant - ref| / (BAR max|ref|) per segment."""
    ref, starts = case["ref"], case["starts"].tolist()
    return [float((mutant[starts[s]:starts[s + 1]] - ref[starts[s]:starts[s + 1]]).abs().max() / (BAR * ref[starts[s]:starts[s + 1]].abs().max()))
            for s in range(len(case["lens"]))]


def packed_margins(case):
    """{mutant name: [(what, margin)]}: how far each mutant of the float64 reference lies from it, in units of the GPU test's bar for the
    segment concerned.  Only (mutant, segment) pairs in which the mutant CAN differ are listed:
      * 'one key more' at every successor row, 'one key fewer' at every diagonal row (row-local: the rest of the segment is the reference);
      * 'sees the row before its start': every segment but the first;
      * 'full attention': every segment of more than one row (a one-row segment has nothing to unmask);
      * 'kv head = head % Hkv': every segment, where that map differs from head // (Hq / Hkv) at all (Hkv > 1)."""
    ref, starts, lens = case["ref"], case["starts"].tolist(), case["lens"]
    Hq, Hkv = case["Hq"], case["Hkv"]
    scale = [BAR * float(ref[starts[s]:starts[s + 1]].abs().max()) for s in range(len(lens))]
    out = {"one key more": [], "one key fewer": []}
    for s, (succ, diag) in enumerate(case["plants"]):
        for r in succ:
            d = float((packed_row(case, s, r, r + 2) - ref[starts[s] + r]).abs().max())
            out["one key more"].append((f"segment {s} (len {lens[s]}) row {r}", d / scale[s]))
        for r in diag:
            d = float((packed_row(case, s, r, r) - ref[starts[s] + r]).abs().max())
            out["one key fewer"].append((f"segment {s} (len {lens[s]}) row {r}", d / scale[s]))
    m = segment_margins(case, packed_ref(case, lead=1))
    out["sees the row before its start"] = [(f"segment {s} (len {lens[s]})", m[s]) for s in range(1, len(lens))]
    m = segment_margins(case, packed_ref(case, causal=False))
    out["full attention"] = [(f"segment {s} (len {lens[s]})", m[s]) for s in range(len(lens)) if lens[s] > 1]
    if Hkv > 1:
        m = segment_margins(case, packed_ref(case, kv_of=[h % Hkv for h in range(Hq)]))
        out["kv head = head % Hkv"] = [(f"segment {s} (len {lens[s]})", m[s]) for s in range(len(lens))]
    return out


# ---- cached prefill (td_attention_bf16, causal, 1 < Sq < Skv) ----------------------------------------------------------------------------------------

PREFILL_SHAPES = [(2, 300), (17, 64), (33, 65), (256, 1029), (257, 320)]
PREFILL_B, PREFILL_HQ, PREFILL_HKV = 2, 12, 2


def prefill_plants(Sq):
    """The planted query rows 0, 31, 32, Sq - 2, Sq - 1 (those that exist) -> (succ rows, diag rows, first-key row).  The two kinds live in different
    kv heads, so they never compete for a key: kv head 0 carries the successor plants (every planted row but the last, whose successor would lie
    behind the cache) and makes key 0 the dominant key of the last query row (so that 'the first key dropped' changes a row completely instead of
    one weight in Skv); kv head 1 carries the diagonal plants."""
    rows = sorted({r for r in (0, 31, 32, Sq - 2, Sq - 1) if 0 <= r < Sq})
    return [r for r in rows if r + 1 < Sq], rows, Sq - 1


_prefill = {}


def prefill_case(Sq, Skv):
    """Operands of one cached-prefill case, batch 2, (Hq, Hkv) = (12, 2): q bf16 [B, Sq, Hq*128]; k, v views [B, Skv, Hkv*128] into one
    cache-shaped buffer [B, Skv + 7, 2*Hkv*128 + 64] (k | v | pad columns; the rows past Skv hold 1e4 and must not be read -- the buffer of
    tests/test_attention_gpu.py's _cache).  Query row i sits at position i + Skv - Sq; its successor plant is key i + Skv - Sq + 1, its diagonal plant
    key i + Skv - Sq.  ref: float64 [B, Sq, Hq*128]."""
    key = (Sq, Skv)
    if key in _prefill:
        return _prefill[key]
    B, Hq, Hkv = PREFILL_B, PREFILL_HQ, PREFILL_HKV
    g = torch.Generator().manual_seed(Sq * 13 + Skv + 5)
    q = torch.randn(B, Sq, Hq * D, generator=g).bfloat16()
    max_len, ld = Skv + 7, 2 * Hkv * D + 64
    buf = torch.randn(B, max_len, ld, generator=g)
    off = Skv - Sq
    succ, diag, first = prefill_plants(Sq)
    for b in range(B):
        for r in succ:
            buf[b, off + r + 1, :D] = _group_sum(q[b, r], Hq, Hkv)[:D]
        buf[b, 0, :D] = _group_sum(q[b, first], Hq, Hkv)[:D]
        for r in diag:
            buf[b, off + r, D:2 * D] = _group_sum(q[b, r], Hq, Hkv)[D:2 * D]
    buf[:, Skv:, :] = 1e4
    buf = buf.bfloat16()
    case = dict(Sq=Sq, Skv=Skv, q=q, buf=buf, k=buf[:, :Skv, :Hkv * D], v=buf[:, :Skv, Hkv * D:2 * Hkv * D], succ=succ, diag=diag, first=first)
    case["ref"] = prefill_ref(case)
    _prefill[key] = case
    return case


def prefill_ref(case, offset_delta=0, first_key=0):
    """float64 causal attention of the Sq query rows against the cache: row i sees keys first_key <= j <= i + Skv - Sq + offset_delta
    (the mutants: offset_delta = +-1, first_key = 1) -> [B, Sq, Hq*128]."""
    Hq, Hkv, Sq, Skv = PREFILL_HQ, PREFILL_HKV, case["Sq"], case["Skv"]
    q, k, v = case["q"], case["k"], case["v"]
    B = q.shape[0]
    qh = q.double().reshape(B, Sq, Hq, D).transpose(1, 2)
    kh = k.double().reshape(B, Skv, Hkv, D).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    vh = v.double().reshape(B, Skv, Hkv, D).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    i = torch.arange(Sq)[:, None] + (Skv - Sq) + offset_delta
    j = torch.arange(Skv)[None, :]
    s = s.masked_fill((j > i) | (j < first_key), float("-inf"))
    o = torch.softmax(s, dim=-1) @ vh
    return o.transpose(1, 2).reshape(B, Sq, Hq * D)


def prefill_margins(case):
    """{mutant: [margin per batch entry]} in units of BAR max|ref| of the batch entry."""
    ref = case["ref"]
    muts = {"causal_offset + 1": prefill_ref(case, offset_delta=1), "causal_offset - 1": prefill_ref(case, offset_delta=-1),
            "first key dropped": prefill_ref(case, first_key=1)}
    return {name: [float((m[b] - ref[b]).abs().max() / (BAR * ref[b].abs().max())) for b in range(ref.shape[0])] for name, m in muts.items()}
