"""Operands, float64 reference and reference mutants of the context-attention case (td_attention_prefix_segments_bf16: packed causal query segments
over key ranges of their own), shared by tests/test_attention_prefix_cases_cpu.py (every mutant lies >= 10x the GPU test's bar from the reference on every
segment it concerns) and tests/test_attention_prefix_gpu.py (the kernel on the same operands).  CPU torch only.

The bar is the one of tests/test_attention_packed_gpu.py, |err| <= 2^-7 max|ref| per segment, and keys are PLANTED as tests/attention_cases_common.py
plants them (k[x] = 3 x the sum of the q heads of a kv head's group makes key x dominant for that query row).  All kv heads of a key row are planted, so one
scheme serves both head configurations.  With off = prefix the position of query row 0:
  * the LAST query row owns its diagonal key (off + q_len - 1, the segment's last key) and, where the segment has two keys or more, key 0 as well: the
    two share the row's weight, so losing either -- causal offset - 1, the first key dropped, the prefix dropped, another slot's rows, an offset taken
    from the longest segment -- moves the row by about half the distance of two value rows;
  * rows 0, 31 and 63 own their successor key (off + r + 1) and rows 33 and 65 their diagonal key (off + r), where they lie at least two rows in front
    of the last (no key is owned twice).
Every cache row outside a segment's key range holds 1e4, so a mutant that reads one (offset + 1 at the last row, the row in front of a slot) is far off too.
"""
import torch

from attention_cases_common import BAR, D, MIN_MARGIN, SCALE, _group_sum  # noqa: F401  (re-exported)

# (q_len, prefix): one-row segments with no, one, a tile less one and a whole tile of prefix; the wave's 32 rows, the 64-key tile and the 256-row workgroup on
# either side, with prefixes that put the diagonal at every phase of a tile; two query tiles behind 513 keys; a short tail behind an image's worth of prefix
CASES = [(1, 0), (1, 1), (1, 63), (1, 64), (2, 300), (31, 1), (32, 32), (33, 255), (64, 64), (65, 191), (255, 1), (256, 256), (257, 63), (300, 513), (16, 1040)]
HEADS = [(4, 2), (7, 1)]
SLOT_ROWS = 1400          # the cache's slot stride: the start of slot s is a multiple of 64 only for s % 8 == 0, and those slots are not used
N_SLOTS = len(CASES) + 3
PAD = 1.0e4


def slots_of(Hq, Hkv):
    """Segment b -> cache slot, scrambled (a different order per head configuration).  Slots 0, 8 and 16 stay unused: the only ones whose start is a
    multiple of the 64-key tile, and every used slot then has a row in front of it."""
    g = torch.Generator().manual_seed(77 + HEADS.index((Hq, Hkv)))
    usable = [s for s in range(N_SLOTS) if s % 8]
    return [usable[i] for i in torch.randperm(len(usable), generator=g).tolist()][:len(CASES)]


def plants(q_len, prefix):
    """-> (successor rows, diagonal rows, first-key row or None) of one segment, as query-row offsets."""
    succ = [r for r in (0, 31, 63) if r <= q_len - 3]
    diag = [r for r in (33, 65) if r <= q_len - 3] + [q_len - 1]
    return succ, diag, (q_len - 1 if prefix + q_len >= 2 else None)


_cases = {}


def prefix_case(Hq, Hkv):
    """One launch's operands: dict with
    qbuf    bf16 [R, Hq*128 + 8]: the packed query rows (pad columns hold 1e4), R = sum of q_len
    cache   bf16 [N_SLOTS * SLOT_ROWS, 2*Hkv*128 + 64]: k | v | pad columns; every row outside a segment's [0, prefix + q_len) holds 1e4
    starts int32 [n + 1], row0 int32 [n] (= slot * SLOT_ROWS), kv_lens int32 [n], slots, q_lens, prefixes
    ref     float64 [R, Hq*128]
    Built once per head configuration and never modified."""
    key = (Hq, Hkv)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(31 * Hq + Hkv)
    q_lens, prefixes = [c[0] for c in CASES], [c[1] for c in CASES]
    starts = [0]
    for n in q_lens:
        starts.append(starts[-1] + n)
    R, QW, KW = starts[-1], Hq * D, Hkv * D
    qbuf = torch.randn(R, QW + 8, generator=g)
    qbuf[:, QW:] = PAD
    qbuf = qbuf.bfloat16()
    slots = slots_of(Hq, Hkv)
    ld = 2 * KW + 64
    cache = torch.full((N_SLOTS * SLOT_ROWS, ld), PAD)
    for b, (n, p) in enumerate(CASES):
        base = slots[b] * SLOT_ROWS
        cache[base:base + p + n, :2 * KW] = torch.randn(p + n, 2 * KW, generator=g)
        succ, diag, first = plants(n, p)
        q = qbuf[starts[b]:starts[b + 1], :QW]
        for r in succ:
            cache[base + p + r + 1, :KW] = _group_sum(q[r], Hq, Hkv)
        for r in diag:
            cache[base + p + r, :KW] = _group_sum(q[r], Hq, Hkv)
        if first is not None:
            cache[base, :KW] = _group_sum(q[first], Hq, Hkv)
    cache = cache.bfloat16()
    case = dict(Hq=Hq, Hkv=Hkv, q_lens=q_lens, prefixes=prefixes, slots=slots, R=R, qbuf=qbuf, cache=cache,
                starts=torch.tensor(starts, dtype=torch.int32), row0=torch.tensor([s * SLOT_ROWS for s in slots], dtype=torch.int32),
                kv_lens=torch.tensor([n + p for n, p in CASES], dtype=torch.int32))
    case["ref"] = prefix_ref(case)
    _cases[key] = case
    return case


def segment_ref(case, b, offset_delta=0, first_key=0, lead=0, base=None, sq_for_offset=None):
    """float64 output of segment b -> [q_len, Hq*128].  Query row i sees keys first_key <= j <= i + (kv_len - Sq) + offset_delta of the rows from
    `base` - lead on (default: the segment's own slot; with lead the rows in front of the slot count as keys 0 .. lead - 1 and shift the rest), Sq = the
    segment's q_len unless sq_for_offset names another.  A row left without a key (a mutant can do that) gives zeros."""
    Hq, Hkv = case["Hq"], case["Hkv"]
    n, p = case["q_lens"][b], case["prefixes"][b]
    KW = Hkv * D
    r0 = int(case["starts"][b])
    a = (int(case["row0"][b]) if base is None else base) - lead
    kv = n + p + lead
    q = case["qbuf"][r0:r0 + n, :Hq * D].double().reshape(n, Hq, D).transpose(0, 1)
    k = case["cache"][a:a + kv, :KW].double().reshape(kv, Hkv, D).transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
    v = case["cache"][a:a + kv, KW:2 * KW].double().reshape(kv, Hkv, D).transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
    sc = q @ k.transpose(1, 2) * SCALE
    i = torch.arange(n)[:, None] + (kv - (n if sq_for_offset is None else sq_for_offset)) + offset_delta
    j = torch.arange(kv)[None, :]
    hidden = (j > i) | (j < first_key)
    sc = sc.masked_fill(hidden, float("-inf"))
    w = torch.softmax(sc, dim=-1)
    w = torch.where(hidden.all(dim=1)[None, :, None], torch.zeros_like(w), w)
    return (w @ v).transpose(0, 1).reshape(n, Hq * D)


def prefix_ref(case):
    return torch.cat([segment_ref(case, b) for b in range(len(CASES))])


def prefix_margins(case):
    """{mutant: [(what, margin)]}: the distance of each mutant of the float64 reference from it in units of BAR max|ref| of the segment, for the segments
    the mutant concerns:
      causal offset + 1               every segment (the last row's extra key is the 1e4 row behind the segment's keys)
      causal offset - 1               segments with two keys or more (the one key of (1, 0) has nothing in front)
      first key dropped               the same
      prefix dropped                  segments with a prefix
      neighbouring slot visible       every segment: the row in front of its slot counts as a key
      row0 of the segment in front    every segment but the first: its keys are read from segment b - 1's slot
      offset from the longest         segments shorter than the longest: c_off = kv_len - max q_len, the formula of the kv_lens form"""
    ref, starts = case["ref"], case["starts"].tolist()
    longest = max(case["q_lens"])
    out = {}

    def add(name, b, got):
        seg = ref[starts[b]:starts[b + 1]]
        out.setdefault(name, []).append((f"segment {b} {CASES[b]}", float((got - seg).abs().max() / (BAR * seg.abs().max()))))

    for b, (n, p) in enumerate(CASES):
        add("causal offset + 1", b, _one_more(case, b))
        if n + p >= 2:
            add("causal offset - 1", b, segment_ref(case, b, offset_delta=-1))
            add("first key dropped", b, segment_ref(case, b, first_key=1))
        if p >= 1:
            add("prefix dropped", b, segment_ref(case, b, first_key=p))
        add("neighbouring slot visible", b, segment_ref(case, b, lead=1))
        if b >= 1:
            add("row0 of the segment in front", b, segment_ref(case, b, base=int(case["row0"][b - 1])))
        if n < longest:
            add("offset from the longest", b, segment_ref(case, b, sq_for_offset=longest))
    return out


def _one_more(case, b):
    """Causal offset + 1: every row sees the key behind its diagonal; for the last row that is the row behind the segment's keys."""
    Hq, Hkv = case["Hq"], case["Hkv"]
    n, p = case["q_lens"][b], case["prefixes"][b]
    KW = Hkv * D
    r0, a, kv = int(case["starts"][b]), int(case["row0"][b]), n + p + 1
    q = case["qbuf"][r0:r0 + n, :Hq * D].double().reshape(n, Hq, D).transpose(0, 1)
    k = case["cache"][a:a + kv, :KW].double().reshape(kv, Hkv, D).transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
    v = case["cache"][a:a + kv, KW:2 * KW].double().reshape(kv, Hkv, D).transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
    sc = q @ k.transpose(1, 2) * SCALE
    sc = sc.masked_fill(torch.arange(kv)[None, :] > torch.arange(n)[:, None] + p + 1, float("-inf"))
    return (torch.softmax(sc, dim=-1) @ v).transpose(0, 1).reshape(n, Hq * D)
