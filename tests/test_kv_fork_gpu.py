"""The KV fork on the GPU (csrc/kv_fork.hip): td_kv_fork_rows on plain byte planes -- every byte of the tensor accounted for -- through the op and
through the C ABI with two planes of different row widths in one call; td_qwen2_fork_slot on the tiny decoder of tests/test_logit_edits_gpu.py for
both cache dtypes, bit for bit against the source slot and against td_qwen2_move_slot copies on a second handle; the refusals.  Every comparison is
an equality."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

V = 4096


def _plane(slots, slot_rows, row_bytes, salt=0):
    """uint8 [slots * slot_rows, row_bytes] with a value that depends on (slot, row, byte) through a hash, so that no two neighbouring 2-, 4-, 8- or
    16-byte pieces of different rows or slots agree."""
    i = torch.arange(slots * slot_rows * row_bytes, dtype=torch.int64)
    return (((i + salt) * 2654435761 >> 7) % 251).to(torch.uint8).view(slots * slot_rows, row_bytes)


def _expected(before, slot_rows, src, dst, n_rows):
    exp = before.clone()
    for d in dst:
        exp[d * slot_rows:d * slot_rows + n_rows] = before[src * slot_rows:src * slot_rows + n_rows]
    return exp


CASES = [(slot_rows, n_rows) for slot_rows, rows in ((5, (0, 1, 5)), (64, (0, 1, 37, 64))) for n_rows in rows]


@pytest.mark.parametrize("row_bytes", [8, 16, 24, 512, 1024, 2048])
def test_fork_rows_touches_exactly_the_destination_rows(hip, row_bytes):
    """slot_rows 5 gives slot starts that are not 16-byte aligned for the 8- and 24-byte rows (40 and 120 bytes per slot: 8-byte pieces); n_rows 0, 1,
    part of a slot (37 of 64: with 2048-byte rows more than one workgroup pass) and all of it; 1, 3 and all other slots as destinations, the source
    below, between and above them.  The whole tensor is compared, so rows >= n_rows of the destinations, the source and the untouched slots count."""
    import thinkdiff.ops  # noqa: F401
    slots = 6
    for slot_rows, n_rows in CASES:
        before = _plane(slots, slot_rows, row_bytes, salt=slot_rows)
        for src, dst in [(0, [3]), (5, [4]), (2, [5, 0, 3]), (4, [0, 2, 5]), (0, [1, 2, 3, 4, 5]), (3, [0, 1, 2, 4, 5]), (5, [0, 1, 2, 3, 4])]:
            x = before.cuda()
            torch.ops.thinkdiff_hip.kv_fork_rows(x, slot_rows, src, dst, n_rows)
            assert torch.equal(x.cpu(), _expected(before, slot_rows, src, dst, n_rows)), (row_bytes, slot_rows, n_rows, src, dst)


@pytest.mark.parametrize("offset", [2, 4, 6, 8, 10, 12, 14])
def test_fork_rows_from_bases_that_are_only_2_4_or_8_byte_aligned(hip, offset):
    """The plane starts `offset` bytes into an allocation: 16-byte slots (width 16) with a head of 16 - offset bytes in 2-byte pieces and a tail of
    `offset` bytes; n_rows 1 (16 bytes: head and tail only, no aligned piece) and 21 (a body between them)."""
    slots, slot_rows, row_bytes = 4, 24, 16
    n = slots * slot_rows * row_bytes
    for n_rows in (1, 21):
        raw = _plane(1, 1, n + 32, salt=offset)[0]
        buf = raw.cuda()
        x = buf[offset:offset + n].view(slots * slot_rows, row_bytes)
        assert x.data_ptr() % 16 == offset
        hip.kv_fork_rows([(x, slot_rows)], 1, [3, 0], n_rows)
        exp = raw.clone()
        exp[offset:offset + n] = _expected(raw[offset:offset + n].view(slots * slot_rows, row_bytes), slot_rows, 1, [3, 0], n_rows).reshape(-1)
        assert torch.equal(buf.cpu(), exp), (offset, n_rows)


def test_two_planes_of_different_row_widths_in_one_call(hip):
    """The e4m3 cache's pair through the C ABI: a byte plane of 512-byte rows and a scale plane of 16-byte rows (fp32), and the odd one: 8-byte rows
    with an odd slot_rows beside 1024-byte rows."""
    for (rb0, dt0), (rb1, dt1), slot_rows, n_rows in [((512, torch.uint8), (16, torch.float32), 64, 40), ((1024, torch.uint8), (8, torch.float32), 5, 3)]:
        slots = 5
        a0, b0 = _plane(slots, slot_rows, rb0, 1), _plane(slots, slot_rows, rb1, 2)
        a, b = a0.cuda(), b0.cuda().view(dt1)
        hip.kv_fork_rows([(a, slot_rows), (b, slot_rows)], 3, [0, 4, 1], n_rows)
        assert torch.equal(a.cpu(), _expected(a0, slot_rows, 3, [0, 4, 1], n_rows))
        assert torch.equal(b.view(torch.uint8).cpu(), _expected(b0, slot_rows, 3, [0, 4, 1], n_rows))


def test_more_planes_and_destinations_than_one_launch_carries(hip):
    """70 planes (64 per launch) and 200 destinations (192 per launch): the argument space is filled in several launches."""
    slot_rows, slots = 2, 201
    before = [_plane(slots, slot_rows, 16 + 8 * (p % 3), p) for p in range(70)]
    xs = [t.cuda() for t in before]
    dst = [d for d in range(slots) if d != 7]
    hip.kv_fork_rows([(x, slot_rows) for x in xs], 7, dst, 2)
    for x, t in zip(xs, before):
        assert torch.equal(x.cpu(), _expected(t, slot_rows, 7, dst, 2))


# ---- the engine --------------------------------------------------------------------------------------------------------------------------------
def _engine(kv, n_slots=6):
    from thinkdiff.models.qwen2_vl import Qwen2VLTextConfig, Qwen2VLTextEngine
    return Qwen2VLTextEngine(Qwen2VLTextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                               intermediate_size=1024, vocab_size=V), max_model_len=64, n_slots=n_slots, kv_cache_dtype=kv).init_random(3, std=0.05)


def _prefill(e, slot, toks):
    return e.forward(e.text_position_ids(len(toks)), torch.tensor(toks, dtype=torch.int32), None, 0, True, True, slot=slot)


PROMPT = [(37 * i + 11) % V for i in range(40)]
OTHER = [(53 * i + 5) % V for i in range(23)]


@pytest.mark.parametrize("kv", ["auto", "fp8"])
def test_engine_fork_slot(hip, kv):
    e, ref = _engine(kv), _engine(kv)
    for eng in (e, ref):
        _prefill(eng, 1, OTHER)
        _prefill(eng, 3, OTHER)
        _prefill(eng, 4, PROMPT)
    others = [[e.read_kv(l, s, 0, 64).clone() for l in range(2)] for s in (1, 3)]
    e.fork_slot(4, [0, 2, 5], 40)
    for l in range(2):
        src = e.read_kv(l, 4, 0, 40)
        for d in (0, 2, 5):
            assert torch.equal(e.read_kv(l, d, 0, 40), src), (kv, l, d)
        for s, keep in zip((1, 3), others):
            assert torch.equal(e.read_kv(l, s, 0, 64), keep[l]), "a slot that is neither source nor destination reads back unchanged"
    for d in (0, 2, 5):
        ref.move_slot(4, d, 40)
    tok, pos = [77] * 4, [[40] * 4] * 3
    hid, lg = e.decode_batch(tok, pos, [40] * 4, slots=[4, 0, 2, 5])
    hid2, lg2 = ref.decode_batch(tok, pos, [40] * 4, slots=[4, 0, 2, 5])
    torch.cuda.synchronize()
    for r in range(1, 4):
        assert torch.equal(hid[r], hid[0]) and torch.equal(lg[r], lg[0]), "the forked sequences decode bit-identically"
    assert torch.equal(hid, hid2) and torch.equal(lg, lg2), "... and as they do from td_qwen2_move_slot copies on a second handle"


@pytest.mark.parametrize("kv", ["auto", "fp8"])
def test_engine_refusals_leave_the_cache_alone(hip, kv):
    e = _engine(kv)
    _prefill(e, 4, PROMPT)
    _prefill(e, 1, OTHER)
    before = [[e.read_kv(l, s, 0, 64).clone() for l in range(2)] for s in range(6)]
    L = hip.lib()

    def fork(src, dst, n):
        arr = (ctypes.c_int * len(dst))(*dst)
        rc = L.td_qwen2_fork_slot(e._h, src, ctypes.cast(arr, ctypes.c_void_p), len(dst), n, hip.stream_ptr())
        return rc, L.td_last_error().decode()

    for (src, dst, n), word in [((4, [0, 2, 0], 40), "slot 0 is given twice"), ((4, [0, 4], 40), "src_slot=4 is among the destinations"),
                                ((4, [0, 2], 65), "len=65"), ((4, [0, 6], 40), "slot 6"), ((6, [0], 40), "slot 6"), ((4, [-1], 40), "slot -1"),
                                ((4, [0], -1), "len=-1")]:
        rc, msg = fork(src, dst, n)
        assert rc == 2 and word in msg, (src, dst, n, rc, msg)
    with pytest.raises(hip.ThinkDiffHipError, match="given twice"):
        e.fork_slot(4, [2, 2], 40)
    torch.cuda.synchronize()
    for s in range(6):
        for l in range(2):
            assert torch.equal(e.read_kv(l, s, 0, 64), before[s][l])
    e.fork_slot(4, [0], 0)      # no rows: nothing happens
    assert torch.equal(e.read_kv(0, 0, 0, 64), before[0][0])
    with pytest.raises(RuntimeError, match="outside the plane's 4 slots"):
        import thinkdiff.ops  # noqa: F401
        torch.ops.thinkdiff_hip.kv_fork_rows(torch.zeros(16, 8, dtype=torch.uint8, device="cuda"), 4, 0, [4], 2)
