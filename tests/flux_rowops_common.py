"""Float64 references and derived per-element bounds for the FLUX step's row kernels (csrc/elementwise.hip), shared by
tests/test_flux_rowops_fp64_gpu.py, tests/test_flux_row_entries_gpu.py and tests/test_norms_gpu.py.

Every reference takes the bf16 inputs in float64 on the CPU and follows the kernel's documented rounding chain, rounding through
`.bfloat16().double()` where the kernel rounds (rbf).  Every bound is built from the reference alone: one bf16 ulp of the reference at
each rounding point, moved through the operations behind it, plus a stated term for the fp32 arithmetic in front of the first
rounding.  No bound comes from what a kernel returned; `record` keeps the measured worst error / bound ratios in
profiles/flux_rowops_fp64_bounds.json as a record only.
"""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "flux_rowops_fp64_bounds.json")


def _ulp(r):
    a = r.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _ref(x, w, b, eps, rms):
    """float64 reference and its per-element tolerance."""
    x = x.double()
    D = x.shape[1]
    wd = w.double() if w is not None else torch.ones(D, dtype=torch.float64)
    if rms:
        rstd = 1.0 / torch.sqrt((x * x).mean(dim=1, keepdim=True) + eps)
        t = (x * rstd).bfloat16().double()
        y = (t * wd).bfloat16().double() if w is not None else t
        tol = _ulp(y) + (wd.abs() * _ulp(t) if w is not None else 0.0)
        return y, tol
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd * wd
    if b is not None:
        y = y + b.double()
    y = y.bfloat16().double()
    return y, _ulp(y) + (D / 64 + 8) * 2.0 ** -24 * x.abs().mean(dim=1, keepdim=True) * rstd * wd.abs()


def _check(got, ref, tol, what):
    """Every element of got within tol of ref; prints and returns the worst error / bound ratio."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    bad = err > tol
    worst = float((err / tol).max())
    print(f"{what}: max error {worst:.3f} x the bound")
    if bad.any():
        i = int(torch.argmax(err / tol))
        r, c = divmod(i, ref.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements beyond the bound; worst row {r} col {c}: got "
                             f"{float(got[r, c]):.6g} ref {float(ref[r, c]):.6g} ({float(err[r, c] / tol[r, c]):.3g} x the bound)")
    return worst


def check_firm(got, ref, firm, what, at_least=0.9):
    """got equals ref by value (+0.0 == -0.0) on every firm element; at least `at_least` of the elements are firm (the fp32 error is
    thousands of times smaller than a bf16 step, so nearly all are: this keeps the comparison from going vacuous)."""
    got = got.double().cpu()
    bad = firm & (got != ref)
    frac = float(firm.double().mean())
    print(f"{what}: {100 * frac:.2f} % of the elements firm")
    assert frac >= at_least, f"{what}: only {100 * frac:.1f} % of the elements are firm"
    if bad.any():
        i = int(torch.argmax(bad.reshape(-1).int()))
        raise AssertionError(f"{what}: {int(bad.sum())} / {int(firm.sum())} firm elements differ from the rounding chain; first at flat index {i}: "
                             f"got {float(got.reshape(-1)[i]):.6g} ref {float(ref.reshape(-1)[i]):.6g}")


def record(key, ratio):
    """Keep the worst error / bound ratio of one test in profiles/flux_rowops_fp64_bounds.json (a record; no bound is read from it)."""
    print(f"{key}: worst error / bound = {ratio:.4f}")
    try:
        with open(RECORD) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    data[key] = round(float(ratio), 4)
    try:
        with open(RECORD, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:      # a read-only checkout still runs the assertions
        pass


def bf(t):
    """One bf16 rounding of a float64 tensor."""
    return t.bfloat16().double()


def tie_margin(v):
    """Distance of a float64 value to the nearest point where its bf16 rounding changes (the middle between two neighbouring bf16 values)."""
    return 0.5 * _ulp(v) - (v - bf(v)).abs()


def bits(t):
    """bf16 tensor -> int16 bit patterns on the CPU (bit-for-bit comparisons, -0.0 and NaN payloads included)."""
    return t.detach().cpu().contiguous().view(torch.int16)


# ---- td_norm_rows_bf16 ----------------------------------------------------------------------------------------------------------

def norm_rows_ref(x, rms, eps, w=None, shift=None, scale=None):
    """float64 reference of td_norm_rows_kernel and its bound.  x bf16 [rows, D]; w bf16 [D] or None; shift / scale bf16 [rows, D]
    (the modulation each row takes, so that the caller decides the split) or None.
      n = (x - mean) * rstd         (rms != 0: mean = 0, rstd = rsqrt(mean(x^2) + eps))
      t0 = bf16(n);  t1 = bf16(t0 * w);  m = bf16(1 + scale);  t2 = bf16(t1 * m);  y = bf16(t2 + shift)
    rms = 2: y = bf16(n * w), one rounding.  Bound: the error that can enter behind each rounding is one ulp of the reference there,
    and it passes through the later multiplications by |w| and |m|:
      ulp(y) + ulp(t2) + |m| ulp(t1) + |m| |w| ulp(t0)  +  F |w m|,   F = (D/64 + 8) 2^-24 mean|x| rstd
    with the terms of absent stages dropped (F: the fp32 row mean, tests/test_norms_gpu.py).

    Third result, `firm`: the elements the kernel must return BIT FOR BIT.  Only the first rounding sees inexact fp32 arithmetic: n carries
    the row mean's error F and a relative error of rstd and of the products of at most (D/128 + 7.5) 2^-24 (the squares' sum has the
    mean's chain and three more roundings per term, rsqrt halves it; v_rsq_f32, x - mean and n = v * rstd add one each), together at most
    d0 = (D/64 + 8) 2^-24 (mean|x| rstd + |n|).  Where n is farther than d0 from a rounding tie, t0 has the reference's bits, and every
    later operand is then a product or a sum of two bf16 values, which fp32 holds exactly (or rounds as the float64 -> fp32 -> bf16
    conversion of the reference does): the rest of the chain is deterministic.  rms = 2 rounds once, n w: firm where that is farther
    than |w| d0 + 2^-24 |n w| from a tie.  A dropped or an added rounding anywhere in the chain shows on the firm elements, which the
    bound alone (it must admit one ulp per rounding point) cannot see."""
    x = x.double()
    D = x.shape[1]
    if rms:
        mean = torch.zeros(x.shape[0], 1, dtype=torch.float64)
    else:
        mean = x.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    n = (x - mean) * rstd
    e0 = (D / 64 + 8) * 2.0 ** -24
    e = (e0 * x.abs().mean(dim=1, keepdim=True) * rstd).expand_as(n)
    if rms == 2:
        assert scale is None
        wd = w.double() if w is not None else torch.ones(D, dtype=torch.float64)
        y = bf(n * wd)
        d = wd.abs() * (e + e0 * n.abs()) + 2.0 ** -24 * (n * wd).abs()
        return y, _ulp(y) + wd.abs() * e, tie_margin(n * wd) > d
    y = bf(n)
    firm = tie_margin(n) > e + e0 * n.abs()
    e = e + _ulp(y)
    if w is not None:
        wd = w.double()
        y = bf(y * wd)
        e = wd.abs() * e + _ulp(y)
    if scale is not None:
        m = bf(1.0 + scale.double())
        y = bf(y * m)
        e = m.abs() * e + _ulp(y)
        y = bf(y + shift.double())
        e = e + _ulp(y)
    return y, e, firm


# ---- td_qk_norm_rope_bf16 / td_qk_norm_rope_premul_bf16, rotate_half = 0 -----------------------------------------------------

def qk_pairs_ref(x, cos, sin, w=None, eps=1e-6, premul=1.0):
    """float64 reference of the interleaved-pair mode on head rows and its bound.  x bf16 [rows, H, 128]; cos / sin fp32 [rows, 128],
    taken as they are, column by column; w bf16 [rows, 128] (the weight each row takes) or None; premul: the fp32 factor (1 for k).
      t0 = bf16(x * rstd);  t1 = bf16(t0 * w)                     rstd = rsqrt(mean(x^2) + eps) over the 128 elements (no w: t1 = x)
      y[2i]   = bf16((t1[2i] cos[2i] - t1[2i+1] sin[2i]) * premul)
      y[2i+1] = bf16((t1[2i+1] cos[2i+1] + t1[2i] sin[2i+1]) * premul)
    Bound, with e(.) = ulp(t1) + |w| ulp(t0) the error that can enter one element (0 without weights), for the pair (a, b):
      ulp(y) + |premul| (|c| e(a) + |s| e(b)) + 4 * 2^-24 |premul| (|a c| + |b s|)
    -- the last term for the fp32 product, fma and premul roundings.

    Third result, `firm`: the elements the kernel must return BIT FOR BIT.  x * rstd carries a relative fp32 error of at most 10 * 2^-24 (the
    128 squares are summed over 8 fmas and 4 butterfly additions, one more fma brings eps: 13 roundings, halved by the rsqrt; v_rsq_f32
    and the product add one each); t0 * w is a product of two bf16 values, exact in fp32; the rotation and the premul carry the last term
    of the bound.  An element is firm when both elements of its pair are farther than the first from a tie at t0 and its own value is
    farther than the last from a tie at y: every rounding then falls as the reference's, whatever the fp32 summation order.  This is
    what tells `bf16(r * premul)` from `bf16(bf16(r) * premul)`, which differ by at most the one ulp the bound must admit."""
    x = x.double()
    rows = x.shape[0]
    c = cos.double().reshape(rows, 1, 128)
    s = sin.double().reshape(rows, 1, 128)
    pm = float(np.float32(premul))
    if w is not None:
        wd = w.double().reshape(rows, 1, 128)
        rstd = 1.0 / torch.sqrt((x * x).mean(dim=-1, keepdim=True) + eps)
        t0 = bf(x * rstd)
        t1 = bf(t0 * wd)
        e = _ulp(t1) + wd.abs() * _ulp(t0)
        firm0 = tie_margin(x * rstd) > 10 * 2.0 ** -24 * (x * rstd).abs()
    else:
        t1 = x
        e = torch.zeros_like(x)
        firm0 = torch.ones_like(x, dtype=torch.bool)
    # partner of element d: d ^ 1; it enters negated at even d
    idx = torch.arange(128) ^ 1
    sign = torch.where(torch.arange(128) % 2 == 0, -1.0, 1.0).double()
    other, e_other = t1[..., idx], e[..., idx]
    v = (t1 * c + sign * other * s) * pm
    y = bf(v)
    f32 = 4 * 2.0 ** -24 * abs(pm) * ((t1 * c).abs() + (other * s).abs())
    tol = _ulp(y) + abs(pm) * (c.abs() * e + s.abs() * e_other) + f32
    return y, tol, firm0 & firm0[..., idx] & (tie_margin(v) > f32)


# ---- td_fill_normal_bf16 / td_fill_normal_from_bf16 ---------------------------------------------------------------------------

def fill_normal_ref(n, seed, std, mean, pair0=0):
    """The documented generator in numpy uint64 / float64: pair p = splitmix64(seed + golden * (pair0 + p + 1)); u1 from its top 24
    bits, u2 from bits 8 .. 31; Box-Muller: element 2p = mean + std r cos(2 pi u2), 2p + 1 = mean + std r sin(2 pi u2), r = sqrt(-2 ln u1).
    The kernel's fp32 constants are taken as fp32 has them: 1 / 16777217.0f is 2^-24 (16777217 is no fp32 number), 2 pi is 6.2831855.
    Returns (value float64 [n], r float64 [n])."""
    pairs = (n + 1) // 2
    with np.errstate(over="ignore"):
        p = np.arange(pairs, dtype=np.uint64) + np.uint64(pair0 + 1)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * p
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u1 = ((z >> np.uint64(40)).astype(np.float64) + 1.0) * float(np.float32(1.0) / np.float32(16777217.0))
    u2 = ((z >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    ang = float(np.float32(6.283185307179586)) * u2
    v = np.stack([mean + std * r * np.cos(ang), mean + std * r * np.sin(ang)], axis=1).reshape(-1)[:n]
    rr = np.repeat(r, 2)[:n]
    return torch.from_numpy(v.copy()), torch.from_numpy(rr.copy())
