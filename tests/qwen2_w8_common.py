"""CPU restatement of the 8-bit weight format of the Qwen2-VL decode engine (include/thinkdiff_hip.h, "8-bit weight stream"), shared by
tests/test_qwen2_w8_cpu.py and tests/test_qwen2_w8_gpu.py.

Format: OCP e4m3 bytes with one power-of-two scale per output row of a Linear weight W[N, K]:
  amax_n = max_k |W[n, k]|;  e_n = the smallest integer with amax_n 2^-e_n <= 448, clamped to [-40, 40], 0 for an all-zero row;
  q[n, k] = e4m3_rne(W[n, k] 2^-e_n);  W^[n, k] = q[n, k] 2^e_n.
Written with torch.frexp (exact exponents, no logarithm) and torch.float8_e4m3fn.  What torch's CPU conversion does is itself checked in
test_qwen2_w8_cpu.py: round to nearest even, 2^-10 -> 0, 1.5 x 2^-9 -> 2^-8, NaN only above the tie at 464 = 448 + 16, which the scale rule excludes.
"""
import torch

E_MIN, E_MAX = -40, 40


def row_exponents(w):
    """e_n of every row of w (any float dtype) as int32."""
    amax = w.float().abs().amax(dim=1)
    m, ex = torch.frexp(amax)                      # amax = m 2^ex, m in [0.5, 1)
    # amax 2^-e <= 448 = 0.875 x 2^9  <=>  e >= ex - 9 when m <= 0.875, else ex - 8
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(E_MIN, E_MAX)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int32)


def quantize_rows(w):
    """-> (q uint8 [N, K] e4m3 bytes, scale fp32 [N] = 2^e_n, w_hat fp32 [N, K] = q 2^e_n, e int32 [N])."""
    wf = w.float()
    e = row_exponents(wf)
    one = torch.ones(wf.shape[0], dtype=torch.float32)
    scale, inv = torch.ldexp(one, e), torch.ldexp(one, -e)
    q = (wf * inv[:, None]).to(torch.float8_e4m3fn)          # the product is exact in fp32 (a power of two): one rounding
    w_hat = q.float() * scale[:, None]
    return q.view(torch.uint8), scale, w_hat, e


def dequantize(q_u8, scale):
    return q_u8.view(torch.float8_e4m3fn).float() * scale[:, None]


def edge_rows(N, K, seed=0):
    """N rows of bf16 weights for the format's corner cases: magnitudes spanning 2^-12 .. 2^12 from row to row, row 0 all zero, row 1 a single
    non-zero, row 2 with a maximum of exactly 448 x 2^3, row 3 just above it (449 rounds to 448 in bf16, so 450 -> 2^4 x ...)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g)
    expo = torch.linspace(-12, 12, N).round()
    w = w * torch.exp2(expo)[:, None]
    w[0] = 0
    if N > 1:
        w[1] = 0
        w[1, K // 3] = -0.37
    if N > 2:
        w[2] = w[2].clamp(-1000, 1000)
        w[2, 5] = 448.0 * 8
    if N > 3:
        w[3] = w[3].clamp(-1000, 1000)
        w[3, K - 1] = -452.0 * 8       # (a bf16 value: 452 = 113 x 4)
    return w.bfloat16()


def ulp_bf16(r):
    """One bf16 ulp at |r| (float64 tensor); 0 and subnormals map to the smallest normal's ulp."""
    a = r.abs().double().clamp_min(2.0 ** -126)
    _, ex = torch.frexp(a)                         # a in [2^(ex-1), 2^ex)
    return torch.ldexp(torch.ones_like(a), ex - 1 - 7)


def sum_bound(K, absdot):
    """Worst-case error of an fp32 sum of K exact products in ANY order: every partial sum is at most absdot = sum_k |x_k w_k| in magnitude, every
    addition rounds by at most 2^-24 of its result, so the total is below K 2^-24 absdot (first order; the second-order term is below 2^-40 of it)."""
    return K * 2.0 ** -24 * absdot


def linear_tol(ref, absdot, K, extra=None):
    """|y - ref| <= ulp_bf16(ref) + K 2^-24 sum_k |x_k w_k| (+ extra: what further rounding points contribute, composed by the caller).
    ref, absdot float64."""
    t = ulp_bf16(ref) + sum_bound(K, absdot)
    return t if extra is None else t + extra
