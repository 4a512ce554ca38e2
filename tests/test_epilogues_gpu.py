"""GEMM epilogue activations on every route, and the gated units, against a float64 CPU reference.

Activation probe: x = identity rows and bias = 0 make every Linear output exact (y[m, n] = W[n, m]), so W carries a grid of
pre-activation values -- every bf16 value in [-12, 12] at a step of 1/64, plus +-20, +-40 and +-0 -- and the epilogue alone
decides the result.  The reference is bf16(act(y)) evaluated in float64.

Tolerance (probe): 1 bf16 ulp of the reference per element, with an absolute floor of 2^-20.  The kernels evaluate the
activation in fp32 (v_exp_f32 / v_rcp_f32 are good to ~1 fp32 ulp) and round once to bf16, so a correct kernel differs from
the float64 value only where that value lies within a few fp32 ulps of a bf16 rounding boundary.  The floor covers the fp32
cancellation in 0.5 x (1 + erf(x / sqrt 2)) for x < -3 (torch's own fp32 GELU shares it): there the exact value is below
~1e-6 and fp32 keeps only a few of its bits.  Where the floor does not apply (|ref| >= 2^-13) at least 99 % of the elements
must be bit-equal to the reference, so a kernel that is consistently one ulp off still fails.

Random-operand epilogue chains (bias -> act -> gate -> residual, each stage rounded to bf16 as in the bf16 torch graph) use
the GEMM tolerance of tests/test_gemm_gpu.py: max |err| <= 2^-7 of the output's largest magnitude; the contraction order is
the only difference from the float64 reference, and that only moves the Linear output's rounding.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = [0, 1, 2, 3, 4]          # TD_ACT_NONE, GELU_TANH, GELU_ERF, SILU, QUICK_GELU
FLOOR = 2.0 ** -20


def _grid():
    k = torch.arange(-768, 769, dtype=torch.float64) / 64
    g = k[k.bfloat16().double() == k]
    return torch.cat([g, torch.tensor([20.0, -20.0, 40.0, -40.0, 0.0, -0.0], dtype=torch.float64)])


GRID = _grid()


def _act64(act, x):
    x = x.double()
    if act == 0:
        return x
    if act == 1:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if act == 2:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == 3:
        return x * torch.sigmoid(x)
    if act == 4:
        return x * torch.sigmoid(1.702 * x)
    raise ValueError(act)


def _ulp(r):
    """One bf16 ulp at |r| (r float64 holding bf16 values); 0 maps to the smallest normal's ulp."""
    a = r.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def _targets(M, N, seed):
    """[M, N] bf16 pre-activation values: the whole probe grid (shuffled), then random picks from it."""
    g = torch.Generator().manual_seed(seed)
    n = M * N
    idx = torch.cat([torch.randperm(len(GRID), generator=g), torch.randint(0, len(GRID), (max(0, n - len(GRID)),), generator=g)])[:n]
    if n >= len(GRID):
        assert len(torch.unique(idx)) == len(GRID)
    return GRID[idx].reshape(M, N).bfloat16()


def _check_act(got, y, act, what, scale=None):
    """got (device bf16) vs bf16(act(y) [* scale]) with the probe tolerance (module docstring)."""
    ref64 = _act64(act, y.double())
    if scale is not None:
        inner = ref64.bfloat16().double()
        ref64 = inner * scale.double()
    ref = ref64.bfloat16()
    got = got.cpu()
    assert got.shape == ref.shape
    g, r = got.double(), ref.double()
    assert torch.isfinite(g).all(), what
    tol = torch.maximum(_ulp(r), torch.full_like(r, FLOOR))
    if scale is not None:
        # one ulp at each rounding point: a near-tie act(g) that fp32 rounds the other way moves the product by |u| ulp(act(g))
        tol = torch.maximum(_ulp(r) + scale.double().abs() * _ulp(inner), FLOOR * scale.double().abs())
    err = (g - r).abs()
    bad = err > tol
    sel = _ulp(r) >= FLOOR
    same = (got.view(torch.int16) == ref.view(torch.int16))[sel].double().mean().item()
    print(f"{what}: act {act}: max error {float((err / tol).max()):.3f} x the bound, bit-equal {same:.5f}")
    if bad.any():
        i = int(torch.argmax(err / tol))
        raise AssertionError(f"{what}: act {act}: {int(bad.sum())} / {bad.numel()} elements beyond 1 bf16 ulp "
                             f"(worst: input {float(y.reshape(-1)[i].double()):.6g} got {float(g.reshape(-1)[i]):.6g} "
                             f"ref {float(r.reshape(-1)[i]):.6g}, {float((err / tol).reshape(-1)[i]):.3g} x the bound)")
    assert same >= 0.99, f"{what}: act {act}: only {same:.4f} of the elements bit-equal to the reference"


def _identity(M, K):
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[torch.arange(M), torch.arange(M)] = 1.0
    return x


def _weights_for(T, K):
    """W [N, K] with W[n, m] = T[m, n]: identity rows times W.T reproduce T."""
    M, N = T.shape
    W = torch.zeros(N, K, dtype=torch.bfloat16)
    W[:, :M] = T.t()
    return W


# ---- activation probe: bf16 routes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("two", [False, True], ids=["one_problem", "two_problems"])
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4])
def test_probe_tile_configs(hip, cfg, two):
    """linear_grouped2 on every tile shape (gemm_bf16.hip: 0 256x256, 1 256x64, 2 32x256, 3 288x192, 4 256x128, -1 the
    planner's choice), with one problem and with two (the second problem reads its own weight and bias)."""
    M0, M1, N, K = 72, 40, 16, 128
    for act in ACTS:
        T0, T1 = _targets(M0, N, 100 + act), _targets(M1, N, 200 + act)
        x0, w0 = _identity(M0, K).cuda(), _weights_for(T0, K).cuda()
        b = torch.zeros(N, dtype=torch.bfloat16, device="cuda")
        y0 = torch.full((M0, N), 7.0, dtype=torch.bfloat16, device="cuda")
        if two:
            x1, w1 = _identity(M1, K).cuda(), _weights_for(T1, K).cuda()
            y1 = torch.full((M1, N), 7.0, dtype=torch.bfloat16, device="cuda")
            hip.linear_grouped2(x0, w0, b, y0, x1, w1, b, y1, act=act, tile_cfg=cfg)
        else:
            hip.linear_grouped2(x0, w0, b, y0, None, None, None, None, act=act, tile_cfg=cfg)
        torch.cuda.synchronize()
        _check_act(y0, T0, act, f"tile cfg {cfg} problem 0")
        if two:
            _check_act(y1, T1, act, f"tile cfg {cfg} problem 1")


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 17, 64, 65, 100])
def test_probe_linear_rows(hip, M):
    """hip.linear at every row count class: M <= 4 the dot-product weight stream, 4 < M <= 64 the matrix-core weight stream
    (csrc/gemv_bf16.hip), M > 64 the tile kernels.  N is chosen so that every probe value appears."""
    N = ((len(GRID) + M - 1) // M + 15) // 16 * 16
    K = max(64, (M + 63) // 64 * 64)
    for act in ACTS:
        T = _targets(M, N, 300 + 7 * M + act)
        x, w = _identity(M, K).cuda(), _weights_for(T, K).cuda()
        y = hip.linear(x, w, torch.zeros(N, dtype=torch.bfloat16, device="cuda"), act=act)
        torch.cuda.synchronize()
        _check_act(y, T, act, f"linear M={M}")


@pytest.mark.parametrize("M,Nh", [(3, 304), (17, 64), (100, 256)])
def test_probe_linear_split(hip, M, Nh):
    """td_linear_split_bf16: columns [0, n_split) -> out0 under act0, the rest -> out1 under act1, every ordered pair of different
    activations, on the dot-product stream (M = 3), the matrix-core stream (M = 17) and the tile kernels (M = 100; n_split is a
    multiple of every tile width)."""
    K = max(64, (M + 63) // 64 * 64)
    for act0 in ACTS:
        for act1 in ACTS:
            if act0 == act1:
                continue
            T = _targets(M, 2 * Nh, 400 + M + 5 * act0 + act1)
            x, w = _identity(M, K).cuda(), _weights_for(T, K).cuda()
            y0 = torch.full((M, Nh + 8), 7.0, dtype=torch.bfloat16, device="cuda")
            y1 = torch.full((M, Nh), 7.0, dtype=torch.bfloat16, device="cuda")
            hip.linear_split(x, w, torch.zeros(2 * Nh, dtype=torch.bfloat16, device="cuda"), y0[:, :Nh], act0, y1, act1, Nh)
            torch.cuda.synchronize()
            _check_act(y0[:, :Nh], T[:, :Nh], act0, f"split M={M} out0")
            _check_act(y1, T[:, Nh:], act1, f"split M={M} out1")
            assert (y0[:, Nh:].cpu().float() == 7.0).all(), "split: out0 written past n_split columns"


def _decompose(T, reps, parts):
    """Integer matrix I [M, N] -> `parts` matrices of representable integers (descending list `reps`) that sum to I."""
    rem = T.clone()
    out = []
    r = torch.tensor(reps, dtype=torch.float64)
    for _ in range(parts):
        a = rem.abs()
        # the largest representable magnitude <= |rem|
        k = torch.searchsorted(r.flip(0), a.reshape(-1), right=True).reshape(a.shape) - 1
        v = r.flip(0)[k.clamp_min(0)] * (k >= 0)
        v = v * torch.sign(rem)
        out.append(v)
        rem = rem - v
    assert (rem == 0).all(), "decomposition needs more parts"
    return out


@pytest.mark.parametrize("kind", ["int8", "fp8"])
def test_probe_8bit(hip, kind):
    """linear_int8 / linear_fp8 with every activation.  Row m of x holds ones in columns m, m + M, ..., W's column block j holds
    part j of 64 y, and every weight column scale is 2^-6: the integer / fp32 contraction and the dequantisation are exact, so
    y = T again."""
    M, N, parts = 72, 16, 21
    K = (M * parts + 127) // 128 * 128
    if kind == "int8":
        reps = list(range(127, 0, -1))
    else:
        allv = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).double()
        reps = sorted({float(v) for v in allv if math.isfinite(v) and v > 0 and v == int(v)}, reverse=True)
    for act in [1, 2, 3, 4]:
        T = _targets(M, N, 500 + act)
        I = T.double().t() * 64                                # [N, M] integers, |I| <= 2560
        W = torch.zeros(N, K, dtype=torch.float64)
        for j, P in enumerate(_decompose(I, reps, parts)):
            W[:, j * M:(j + 1) * M] = P
        X = torch.zeros(M, K, dtype=torch.float64)
        for j in range(parts):
            X[torch.arange(M), j * M + torch.arange(M)] = 1.0
        xs = torch.ones(M, dtype=torch.float32, device="cuda")
        ws = torch.full((N,), 2.0 ** -6, dtype=torch.float32, device="cuda")
        b = torch.zeros(N, dtype=torch.bfloat16, device="cuda")
        if kind == "int8":
            xq, wq = X.to(torch.int8).cuda(), W.to(torch.int8).cuda()
            assert torch.equal(wq.cpu().double(), W)
            y = hip.linear_int8(xq, xs, wq, ws, b, act=act)
        else:
            xq = X.to(torch.float8_e4m3fn).view(torch.uint8).cuda()
            wq = W.to(torch.float8_e4m3fn)
            assert torch.equal(wq.double(), W)
            y = hip.linear_fp8(xq, xs, wq.view(torch.uint8).cuda(), ws, b, act=act)
        torch.cuda.synchronize()
        _check_act(y, T, act, kind)


# ---- random operands: the whole epilogue chain -----------------------------------------------------------------------

def _chain64(y, b, act, gate, res):
    """float64 chain with the bf16 graph's rounding points: Linear output, activation, gate, residual each round."""
    y = y.double()
    if b is not None:
        y = y + b.double()
    y = y.bfloat16().double()
    if act:
        y = _act64(act, y).bfloat16().double()
    if gate is not None:
        y = (y * gate.double()).bfloat16().double()
    if res is not None:
        y = (y + res.double()).bfloat16().double()
    return y


def _close(got, ref, tol=2.0 ** -7, what=""):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    err = ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()
    print(f"{what}: max rel-to-scale error {err:.3e} (bound {tol:.3e})")
    assert err < tol, f"{what}: max rel-to-scale error {err:.3e}"


@pytest.mark.parametrize("route", ["tile", "grouped", "skinny_dot", "skinny_mfma", "int8", "fp8"])
def test_epilogue_chain_random(hip, route):
    """bias -> act -> gate -> residual on random operands, for every activation with and without the gate / residual stages."""
    M = {"tile": 130, "grouped": 96, "skinny_dot": 3, "skinny_mfma": 17, "int8": 130, "fp8": 130}[route]
    N, K = 256, 512
    for act in ACTS:
        for stages in ["bias", "gate", "gate_res", "res"]:
            g = torch.Generator().manual_seed(1000 + 10 * act + len(stages) + M)
            x = torch.randn(M, K, generator=g).bfloat16()
            w = (torch.randn(N, K, generator=g) * 0.08).bfloat16()
            b = torch.randn(N, generator=g).bfloat16()
            gate = torch.randn(N, generator=g).bfloat16() if "gate" in stages else None
            res = torch.randn(M, N, generator=g).bfloat16() if "res" in stages else None
            dev = lambda t: None if t is None else t.cuda()
            what = f"{route} act {act} {stages}"
            if route in ("int8", "fp8"):
                xq, xs = (hip.quant_rows_int8 if route == "int8" else hip.quant_rows_fp8)(x.cuda())
                wq, ws = (hip.quant_rows_int8 if route == "int8" else hip.quant_rows_fp8)(w.cuda())
                fn = hip.linear_int8 if route == "int8" else hip.linear_fp8
                y = fn(xq, xs, wq, ws, b.cuda(), act=act, gate=dev(gate), res=dev(res))
                if route == "int8":
                    xd, wd = xq.cpu().double(), wq.cpu().double()
                else:
                    xd, wd = xq.cpu().view(torch.float8_e4m3fn).double(), wq.cpu().view(torch.float8_e4m3fn).double()
                y64 = (xd @ wd.t()) * xs.cpu().double()[:, None] * ws.cpu().double()[None, :]
            elif route == "grouped":
                x1 = torch.randn(M // 2, K, generator=g).bfloat16()
                res1 = torch.randn(M // 2, N, generator=g).bfloat16() if res is not None else None
                y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda") if res is None else res.cuda()
                y1 = torch.empty(M // 2, N, dtype=torch.bfloat16, device="cuda") if res1 is None else res1.cuda()
                hip.linear_grouped2(x.cuda(), w.cuda(), b.cuda(), y, x1.cuda(), w.cuda(), b.cuda(), y1, act=act,
                                    gate0=dev(gate), res0=None if res is None else y, gate1=dev(gate),
                                    res1=None if res1 is None else y1, tile_cfg=0)
                torch.cuda.synchronize()
                _close(y1, _chain64(x1.double() @ w.double().t(), b, act, gate, res1), what=what + " problem 1")
                y64 = x.double() @ w.double().t()
            else:
                y = hip.linear(x.cuda(), w.cuda(), b.cuda(), act=act, gate=dev(gate), res=dev(res))
                y64 = x.double() @ w.double().t()
            torch.cuda.synchronize()
            _close(y, _chain64(y64, b, act, gate, res), what=what)


# ---- gated units -------------------------------------------------------------------------------------------------------

def _gate_up(rows, I, seed):
    g = torch.Generator().manual_seed(seed)
    gate = _targets(1, rows * I, seed).reshape(rows, I)
    up = torch.randn(rows, I, generator=g).bfloat16()
    return gate, up, torch.cat([gate, up], dim=1).contiguous()


def _silu_mul(hip, gu):
    rows, two_i = gu.shape
    out = torch.empty(rows, two_i // 2, dtype=torch.bfloat16, device=gu.device)
    hip.check(hip.lib().td_silu_mul_bf16(hip.ptr(gu), hip.ptr(out), rows, two_i // 2, hip.stream_ptr()))
    return out


@pytest.mark.parametrize("act", ACTS + ["silu_mul"])
@pytest.mark.parametrize("rows,I", [(1, 8), (3, 1024), (257, 5120), (1, 5120), (257, 8), (3, 8)])
def test_glu_and_silu_mul(hip, rows, I, act):
    """out = bf16(bf16(act(g)) * u) for glu_mul under every activation and for td_silu_mul_bf16 (SiLU).  The probe grid sits in the
    gate half, u is random.  Bound: one bf16 ulp at each of the two rounding points, i.e. ulp(out) + |u| ulp(bf16(act(g))), floor
    2^-20 |u| (the module docstring's floor through the exact bf16 x bf16 product).  The inner term is needed: at g = 5.9375 the
    float64 SiLU lies 5e-6 above a bf16 tie, fp32 lands below it, and the product then differs by two output ulps."""
    gate, up, gu = _gate_up(rows, I, rows * 31 + I)
    d = gu.cuda()
    if act == "silu_mul":
        _check_act(_silu_mul(hip, d), gate, 3, f"silu_mul rows={rows} I={I}", scale=up)
    else:
        _check_act(hip.glu_mul(d, act), gate, act, f"glu_mul rows={rows} I={I}", scale=up)


# ---- refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("code", [5, -1, 99])
def test_unknown_activation_codes_are_refused(hip, code):
    """Activation codes outside TD_ACT_NONE .. TD_ACT_QUICK_GELU (0 .. 4) are an argument error on every route, not a silent
    fallback (QuickGELU on the tile kernels, identity on the weight stream, SiLU in glu_mul)."""
    E = hip.ThinkDiffHipError
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    for M in (1, 17, 100):
        with pytest.raises(E, match="activation"):
            hip.linear(z(M, 128), z(64, 128), act=code)
        with pytest.raises(E, match="activation"):
            hip.linear_split(z(M, 128), z(64, 128), None, z(M, 32), 0, z(M, 32), code, 32)
    with pytest.raises(E, match="activation"):
        hip.linear_grouped2(z(100, 128), z(64, 128), None, z(100, 64), None, None, None, None, act=code, tile_cfg=0)
    with pytest.raises(E, match="activation"):
        hip.glu_mul(z(4, 64), code)
    torch.cuda.synchronize()
