"""The FLUX step's two heavy row kernels against float64 at their edges: the adaLN row norm (td_norm_rows_kernel<NCH>, all eight
instantiations) and the per-head QK-RMSNorm + RoPE in interleaved-pair mode (td_qk_norm_rope_kernel, rotate_half = 0), the latter also
through td_qk_norm_rope_premul_bf16, which folds the attention scale into q as the engine does.

References and bounds: tests/flux_rowops_common.py (float64 on the CPU along the kernel's rounding chain; one bf16 ulp of the reference
per rounding point, moved through the later operations, plus a stated fp32 term).  Every element is compared; sentinel columns are
compared bit for bit.  The worst error / bound ratio of every test goes to profiles/flux_rowops_fp64_bounds.json.

A bound that admits one ulp per rounding point cannot see a rounding that is dropped or moved (the result only gets closer to float64):
`bf16(bf16(r) * premul)` against `bf16(r * premul)`, or `t0 * w` left unrounded in front of the modulation, stay inside it.  So the
references also mark the FIRM elements -- those whose every pre-rounding value is farther from a rounding tie than the fp32 arithmetic in
front of it can be off -- and on these (98 % and more of every case) the kernel must return the reference's bits.
"""
import math

import numpy as np
import pytest
import torch

import flux_rowops_common as C
from oracle import flux_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -3.0


# ---- td_norm_rows_bf16 ----------------------------------------------------------------------------------------------------------

def _splits(rows):
    s = {0, 1, rows - 1, rows}
    if rows == 9:
        s.add(5)            # cuts the second 4-row block
    return sorted(v for v in s if 0 <= v <= rows)


# (rms, weight, modulation, eps)
NORM_MODES = [(0, False, False, 1e-6), (0, False, True, 1e-6), (0, False, True, 1e-5), (1, True, False, 1e-6), (1, True, True, 1e-5),
              (0, True, True, 1e-6), (2, True, False, 1e-6), (2, True, False, 1e-5)]


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("D", [512, 1024, 1536, 2048, 2560, 3072, 3584, 4096])
def test_norm_rows_vs_float64(hip, D, rows):
    """Every element within the derived bound of float64, and bit for bit where the fp32 statistics cannot move a rounding (the firm elements
    of flux_rowops_common.norm_rows_ref: a dropped or added rounding shows there).  Every instantiation (NCH = D / 512 = 1 .. 8) in every
    mode: LayerNorm plain, + modulation, RMS + w, RMS + w + modulation, LayerNorm + w + modulation, rms = 2 + w; both eps; every split
    (0, 1, rows - 1, rows, and 5 of 9 rows, which cuts a 4-row block) with A / B modulations an offset of 1.5 apart (a row taking the wrong part is off by hundreds of times the bound); scaleB = shiftB = None
    (all rows take A).  x and y are strided and y's pad columns must keep their bits.  A block holds 4 rows, one wave each."""
    g = torch.Generator().manual_seed(D * 31 + rows)
    ldx, ldy = D + 24, D + 16
    xs = (torch.randn(rows, ldx, generator=g) * 1.5 + 0.3).bfloat16()
    w = (1.0 + 0.3 * torch.randn(D, generator=g)).bfloat16()
    shA, scA = (0.3 * torch.randn(D, generator=g)).bfloat16(), (0.3 * torch.randn(D, generator=g)).bfloat16()
    shB, scB = (1.5 + 0.3 * torch.randn(D, generator=g)).bfloat16(), (-1.5 + 0.3 * torch.randn(D, generator=g)).bfloat16()
    x = xs[:, :D]
    xd = xs.cuda()[:, :D]
    dev = {k: v.cuda() for k, v in dict(w=w, shA=shA, scA=scA, shB=shB, scB=scB).items()}
    worst = 0.0

    def run(rms, use_w, eps, what, **mod):
        yfull = torch.full((rows, ldy), SENTINEL, dtype=torch.bfloat16, device="cuda")
        hip.norm_rows(xd, out=yfull[:, :D], rms=rms, eps=eps, w=dev["w"] if use_w else None, **mod)
        torch.cuda.synchronize()
        assert (yfull[:, D:].cpu().float() == SENTINEL).all(), what + ": pad columns of y written"
        return yfull[:, :D]

    for rms, use_w, use_mod, eps in NORM_MODES:
        ww = w if use_w else None
        tag = f"norm_rows D={D} rows={rows} rms={rms} w={use_w} mod={use_mod} eps={eps}"
        if not use_mod:
            ref, tol, firm = C.norm_rows_ref(x, rms, eps, ww)
            y = run(rms, use_w, eps, tag)
            worst = max(worst, C._check(y, ref, tol, tag))
            C.check_firm(y, ref, firm, tag)
            continue
        for split in _splits(rows):
            partB = (torch.arange(rows) >= split)[:, None]
            ref, tol, firm = C.norm_rows_ref(x, rms, eps, ww, shift=torch.where(partB, shB, shA), scale=torch.where(partB, scB, scA))
            y = run(rms, use_w, eps, tag, split=split, shiftA=dev["shA"], scaleA=dev["scA"], shiftB=dev["shB"], scaleB=dev["scB"])
            worst = max(worst, C._check(y, ref, tol, f"{tag} split={split}"))
            C.check_firm(y, ref, firm, f"{tag} split={split}")
        # no B set: every row takes A, whatever the split
        split = min(1, rows - 1)
        ref, tol, firm = C.norm_rows_ref(x, rms, eps, ww, shift=shA.expand(rows, D), scale=scA.expand(rows, D))
        y = run(rms, use_w, eps, tag, split=split, shiftA=dev["shA"], scaleA=dev["scA"])
        worst = max(worst, C._check(y, ref, tol, f"{tag} split={split} B=None"))
        C.check_firm(y, ref, firm, f"{tag} split={split} B=None")
    assert worst <= 1.0
    C.record(f"norm_rows[D={D},rows={rows}]", worst)


def test_norm_rows_refusals(hip):
    """D that is no multiple of 512, D beyond the eight instantiations, a row stride that is no multiple of 8 and a scale without a shift
    are argument errors: nothing is launched and y keeps its bits."""
    buf = torch.zeros(4, 4640, dtype=torch.bfloat16, device="cuda")
    y = torch.full((4, 4640), SENTINEL, dtype=torch.bfloat16, device="cuda")
    sc = torch.zeros(4640, dtype=torch.bfloat16, device="cuda")
    for what, kw, D, ld in [("D=520", {}, 520, 4640), ("D=4608", {}, 4608, 4640), ("ldx % 8", {}, 512, 4636),
                            ("scale without shift", dict(scaleA=sc), 512, 4640), ("shift without scale", dict(shiftA=sc), 512, 4640)]:
        x = buf.view(-1)[: 4 * ld].view(4, ld)[:, :D]
        with pytest.raises(hip.ThinkDiffHipError, match="td_norm_rows"):
            hip.norm_rows(x, out=y[:, :D], **kw)
    with pytest.raises(hip.ThinkDiffHipError, match="td_norm_rows"):        # ldy % 8
        hip.norm_rows(buf[:, :512], out=y.view(-1)[: 4 * 4636].view(4, 4636)[:, :512])
    torch.cuda.synchronize()
    assert (y.cpu().float() == SENTINEL).all()


# ---- td_qk_norm_rope_bf16 / td_qk_norm_rope_premul_bf16, rotate_half = 0 -----------------------------------------------------

ENGINE_PREMUL = float(np.float32(128 ** -0.5) * np.float32(1.4426950408889634))      # flux_engine.hip: scale * log2(e), in fp32
PREMULS = [1.0, ENGINE_PREMUL, 2.0]
# (Hq, Hk, k in front of q): 16 lanes own a head row and a block makes 16 head units per pass of its `u += 16` loop -- 2, 7, 16 (one pass
# exactly), 17 (one unit in the second pass), 48 (three passes) and 33 units (third pass with one unit, no k at all)
QK_SHAPES = [(1, 1, False), (5, 2, False), (5, 2, True), (8, 8, False), (9, 8, False), (24, 24, False), (33, 0, False)]


def _layout(Hq, Hk, k_first):
    """Columns: 8 sentinel | first block | 24 sentinel | second block | 136 sentinel (a v head and a tail).  Returns (ld, q_col, k_col)."""
    a, b = (Hk, Hq) if k_first else (Hq, Hk)
    c0 = 8
    c1 = c0 + a * 128 + 24
    ld = c1 + b * 128 + 136
    return (ld, c1, c0) if k_first else (ld, c0, c1)


def _flux_ids(rows):
    """Text rows at id 0, then image ids (0, y, x) and, as Kontext appends them, reference-image ids (1, y, x) with their own offsets."""
    n_txt = rows // 3
    n_img = (rows - n_txt + 1) // 2
    n_ref = rows - n_txt - n_img
    img = R.latent_image_ids(5, 4)[:n_img] + torch.tensor([0.0, 5.0, 9.0])
    ref = R.latent_image_ids(5, 4)[:n_ref] + torch.tensor([1.0, 2.0, 40.0])
    return torch.cat([torch.zeros(n_txt, 3), img, ref])


def _qk_input(rows, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, ld, generator=g) * 1.5).bfloat16()
    assert (x != 0).all()
    return x


def _heads(t, col, H):
    return t[:, col: col + H * 128].reshape(t.shape[0], H, 128)


def _outside_mask(ld, Hq, Hk, q_col, k_col):
    m = torch.ones(ld, dtype=torch.bool)
    m[q_col: q_col + Hq * 128] = False
    m[k_col: k_col + Hk * 128] = False
    return m


def _check_qk(out, src, Hq, Hk, q_col, k_col, cos, sin, wq, wk, premul, what):
    """q and k heads of `out` against float64 (wq / wk: per-row weights [rows, 128] or None): every element within the bound, the firm ones
    (flux_rowops_common.qk_pairs_ref) bit for bit; everything else bit-equal to src."""
    rows, ld = src.shape
    outside = _outside_mask(ld, Hq, Hk, q_col, k_col)
    assert torch.equal(C.bits(out)[:, outside], C.bits(src)[:, outside]), what + ": a column outside the q and k heads was written"
    worst = 0.0
    for name, col, H, w, pm in (("q", q_col, Hq, wq, premul), ("k", k_col, Hk, wk, 1.0)):
        if H == 0:
            continue
        ref, tol, firm = C.qk_pairs_ref(_heads(src, col, H), cos, sin, w, 1e-6, pm)
        got = _heads(out.cpu(), col, H).reshape(rows, -1)
        worst = max(worst, C._check(got, ref.reshape(rows, -1), tol.reshape(rows, -1), f"{what} {name}"))
        C.check_firm(got, ref.reshape(rows, -1), firm.reshape(rows, -1), f"{what} {name}")
    return worst


@pytest.mark.parametrize("rows", [1, 2, 19])
@pytest.mark.parametrize("Hq,Hk,k_first", QK_SHAPES)
def test_qk_norm_rope_pairs_vs_float64(hip, Hq, Hk, k_first, rows):
    """The FLUX mode on real FLUX tables: four distinct norm weights with split 0, 1 and rows, and no weights at all; q_premul 1, the
    engine's 128^-0.5 log2(e) and 2.  q and k blocks are not adjacent (gap and tail columns, k in front of q in one shape) and every
    column outside them keeps its bits.  Under a premul the k heads equal those of the premul = 1 run bit for bit, and at premul = 1 the
    new entry equals td_qk_norm_rope_bf16 bit for bit."""
    ld, q_col, k_col = _layout(Hq, Hk, k_first)
    src = _qk_input(rows, ld, Hq * 1000 + Hk * 10 + rows)
    cos, sin = R.rope_tables(_flux_ids(rows))
    cd, sd = cos.cuda(), sin.cuda()
    g = torch.Generator().manual_seed(7)
    w4 = [(1.0 + 0.3 * torch.randn(128, generator=g)).bfloat16() for _ in range(4)]       # qA, kA, qB, kB
    w4d = [t.cuda() for t in w4]
    worst = 0.0
    for split in sorted({0, 1, rows}) + [None]:
        if split is None:
            kw, wq, wk, s = {}, None, None, 0
        else:
            kw = dict(split=split, wqA=w4d[0], wkA=w4d[1], wqB=w4d[2], wkB=w4d[3])
            partB = (torch.arange(rows) >= split)[:, None]
            wq, wk, s = torch.where(partB, w4[2], w4[0]), torch.where(partB, w4[3], w4[1]), split
        tag = f"qk_norm_rope Hq={Hq} Hk={Hk} k_first={k_first} rows={rows} weights={split is not None} split={s}"
        k_plain = None
        for pm in PREMULS:
            out = hip.qk_norm_rope_premul(src.cuda(), Hq, Hk, q_col, k_col, cd, sd, q_premul=pm, **kw)
            torch.cuda.synchronize()
            worst = max(worst, _check_qk(out, src, Hq, Hk, q_col, k_col, cos, sin, wq, wk, pm, f"{tag} premul={pm:.4g}"))
            k_now = C.bits(out)[:, k_col: k_col + Hk * 128]
            if pm == 1.0:
                k_plain = k_now
                old = hip.qk_norm_rope(src.cuda(), Hq, Hk, q_col, k_col, cd, sd, **kw)
                torch.cuda.synchronize()
                assert torch.equal(C.bits(old), C.bits(out)), tag + ": premul = 1 differs from td_qk_norm_rope_bf16"
            else:
                assert torch.equal(k_now, k_plain), f"{tag}: premul={pm:.4g} changed the k heads"
    assert worst <= 1.0
    C.record(f"qk_norm_rope_pairs[Hq={Hq},Hk={Hk},k_first={int(k_first)},rows={rows}]", worst)


@pytest.mark.parametrize("Hq,Hk", [(5, 2), (9, 8), (33, 0)])
def test_qk_rope_pairs_structure_exact(hip, Hq, Hk):
    """No norm weights, no tolerance: cos = 1, sin = 0 returns the input's bits; cos = 0, sin = 1 gives y[2i] = -x[2i+1], y[2i+1] = x[2i];
    with a table whose every (row, column) entry is different, exchanging two rows of the table and of the input exchanges those two
    rows of the output and leaves the others alone (each row reads its own table row)."""
    rows = 6
    ld, q_col, k_col = _layout(Hq, Hk, False)
    src = _qk_input(rows, ld, Hq + Hk)
    one, zero = torch.ones(rows, 128, device="cuda"), torch.zeros(rows, 128, device="cuda")
    out = hip.qk_norm_rope_premul(src.cuda(), Hq, Hk, q_col, k_col, one, zero)
    torch.cuda.synchronize()
    # (the input holds no zero: x * 1 -+ x' * 0 = x and x * 0 -+ x' * 1 = -+x' to the bit for every finite non-zero x, x')
    assert torch.equal(C.bits(out), C.bits(src)), "identity rotation changed bits"
    out = hip.qk_norm_rope_premul(src.cuda(), Hq, Hk, q_col, k_col, zero, one).cpu()
    torch.cuda.synchronize()
    want = src.clone()
    for col, H in ((q_col, Hq), (k_col, Hk)):
        blk = src[:, col: col + H * 128].reshape(rows, H * 64, 2)
        want[:, col: col + H * 128] = torch.stack([-blk[..., 1], blk[..., 0]], dim=-1).reshape(rows, H * 128)
    assert torch.equal(C.bits(out), C.bits(want)), "quarter-turn rotation is not (-x[2i+1], x[2i])"

    g = torch.Generator().manual_seed(11)
    ang = torch.rand(rows, 128, generator=g) * 6.0
    cos, sin = torch.cos(ang), torch.sin(ang)
    out1 = hip.qk_norm_rope_premul(src.cuda(), Hq, Hk, q_col, k_col, cos.cuda(), sin.cuda(), q_premul=ENGINE_PREMUL)
    torch.cuda.synchronize()
    worst = _check_qk(out1, src, Hq, Hk, q_col, k_col, cos, sin, None, None, ENGINE_PREMUL, f"qk_rope distinct table Hq={Hq} Hk={Hk}")
    assert worst <= 1.0
    perm = torch.tensor([0, 4, 2, 3, 1, 5])
    out2 = hip.qk_norm_rope_premul(src[perm].cuda(), Hq, Hk, q_col, k_col, cos[perm].cuda(), sin[perm].cuda(), q_premul=ENGINE_PREMUL)
    torch.cuda.synchronize()
    assert torch.equal(C.bits(out2), C.bits(out1)[perm]), "a row did not take its own table row"
    # ... and the table rows do matter: rows 1 and 4 under each other's table rows differ from out1
    out3 = hip.qk_norm_rope_premul(src.cuda(), Hq, Hk, q_col, k_col, cos[perm].cuda(), sin[perm].cuda(), q_premul=ENGINE_PREMUL)
    torch.cuda.synchronize()
    same = (C.bits(out3) == C.bits(out1)).all(dim=1)
    assert same.tolist() == [True, False, True, True, False, True]
    C.record(f"qk_rope_pairs_distinct_table[Hq={Hq},Hk={Hk}]", worst)


def test_qk_norm_rope_premul_refusals(hip):
    """The new entry refuses what td_qk_norm_rope_bf16 refuses, before any launch."""
    src = _qk_input(2, 520, 1)
    d = src.cuda()
    t = torch.ones(2, 128, device="cuda")
    L = hip.lib()
    for what, args in [("rotate_half=3", (hip.ptr(d), 520, 2, 1, 1, 0, 128, hip.ptr(t), hip.ptr(t), 0, None, None, None, None, 1e-6, 3, 1.0, None)),
                       ("q_col % 8", (hip.ptr(d), 520, 2, 1, 1, 4, 136, hip.ptr(t), hip.ptr(t), 0, None, None, None, None, 1e-6, 0, 1.0, None)),
                       ("Hq = 0", (hip.ptr(d), 520, 2, 0, 1, 0, 128, hip.ptr(t), hip.ptr(t), 0, None, None, None, None, 1e-6, 0, 1.0, None))]:
        assert L.td_qk_norm_rope_premul_bf16(*args) == 2, what
        assert b"td_qk_norm_rope" in L.td_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(C.bits(d), C.bits(src))
    assert math.isclose(ENGINE_PREMUL, 128 ** -0.5 * math.log2(math.e), rel_tol=1e-6)
