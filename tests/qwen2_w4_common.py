"""CPU restatement of the MXFP4 weight format of the Qwen2-VL decode engine (include/thinkdiff_hip.h, "4-bit weight stream"), shared by
tests/test_qwen2_w4_cpu.py and tests/test_qwen2_w4_gpu.py.

Format: OCP MXFP4 -- e2m1 elements under one e8m0 power-of-two scale per block of 32 consecutive k of a row of W[N, K], K % 32 == 0:
  amax = max |w| over the block;  e = floor(log2(amax)) - 2, clamped to [-64, 64], 0 for an all-zero block;
  q = e2m1_rne(w 2^-e): nearest value of the grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, beyond 6 -> 6; a sign bit, kept by -0;
  W^ = q 2^e.  packed[n, j] = code(2j) | code(2j + 1) << 4;  scales[n, b] = e + 127.
Written with torch.frexp (exact exponents, no logarithm), a nearest-value search over the grid and a 16-entry table -- not with the thresholds the
kernel compares against.  The functions run on any device (the GPU tests dequantise large random byte matrices there).
"""
import torch

from qwen2_w8_common import linear_tol, sum_bound, ulp_bf16  # noqa: F401  (the analytic bound is the same bound: exact products, fp32 sum in some order)

BLOCK = 32
E_MIN, E_MAX = -64, 64
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
TABLE = GRID + tuple(-g for g in GRID)          # value of every 4-bit code (code 8 is -0.0)
_EVEN_FIRST = (0, 2, 4, 6, 1, 3, 5, 7)          # argmin returns the first minimum: a tie between two neighbours goes to the even code


def block_exponents(w):
    """e of every block of w [N, K] (any float dtype) as int32 [N, K / 32]."""
    N, K = w.shape
    amax = w.float().abs().view(N, K // BLOCK, BLOCK).amax(dim=2)
    _, ex = torch.frexp(amax)                      # amax = m 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = (ex - 3).clamp(E_MIN, E_MAX)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int32)


def e2m1_codes(v):
    """4-bit codes (uint8) of scaled values v (fp32): nearest grid value, ties to the even code, saturated at 6, sign bit from v's own (so -0 keeps it)."""
    a = v.abs().double().clamp_max(6.0)
    order = torch.tensor(_EVEN_FIRST, device=v.device)
    cand = torch.tensor([GRID[i] for i in _EVEN_FIRST], dtype=torch.float64, device=v.device)
    code = order[(a.unsqueeze(-1) - cand).abs().argmin(dim=-1)]
    return (code + 8 * torch.signbit(v).long()).to(torch.uint8)


def pack(codes):
    """codes uint8 [N, K] -> packed uint8 [N, K / 2], element 2j in the low nibble of byte j."""
    return codes[:, 0::2] | (codes[:, 1::2] << 4)


def unpack(packed):
    out = torch.empty(packed.shape[0], packed.shape[1] * 2, dtype=torch.uint8, device=packed.device)
    out[:, 0::2] = packed & 15
    out[:, 1::2] = packed >> 4
    return out


def dequantize(packed, scales):
    """packed [N, K / 2], scales [N, K / 32] -> W^ fp32 [N, K] (the 16-entry table times 2^(scale - 127))."""
    table = torch.tensor(TABLE, dtype=torch.float32, device=packed.device)
    v = table[unpack(packed).long()]
    e = scales.to(torch.int32) - 127
    return torch.ldexp(v, e.repeat_interleave(BLOCK, dim=1))


def quantize_blocks(w, bump=0):
    """-> (packed uint8 [N, K / 2], scales uint8 [N, K / 32], w_hat fp32 [N, K], e int32 [N, K / 32]).  bump: a foreign scale rule whose exponents are
    `bump` higher than the OCP rule's (unclamped blocks only make sense)."""
    wf = w.float()
    e = block_exponents(wf) + bump
    scaled = torch.ldexp(wf, -e.repeat_interleave(BLOCK, dim=1))          # exact in fp32 (a power of two): one rounding, in e2m1_codes
    packed = pack(e2m1_codes(scaled))
    scales = (e + 127).to(torch.uint8)
    return packed, scales, dequantize(packed, scales), e


def bf16_bits(t):
    """The bit patterns of t as bf16 (int16): what torch.equal on values cannot see is the sign of a zero."""
    return t.to(torch.bfloat16).contiguous().view(torch.int16)


TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)                 # at e = 0 -> 0, 1, 1, 2, 2, 4, 4
TIES_ROUNDED = (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0)
N_EDGE = 12


def _edge(i, g):
    """Edge block i (fp32 [32]); every value is a bf16 value."""
    b = torch.zeros(BLOCK)
    small = (torch.randn(BLOCK, generator=g) * 0.5).bfloat16().float().clamp(-1.5, 1.5)
    if i == 0:      # the seven ties and the saturating 7 at e = 0 (amax = 7), both signs
        vals = list(TIES) + [7.0]
        b[:8] = torch.tensor(vals)
        b[8:16] = -torch.tensor(vals)
        b[16:] = small[16:]
    elif i == 1:    # a zero block
        pass
    elif i == 2:    # a single non-zero
        b[11] = -0.37
    elif i == 3:    # -0 among ordinary values
        b = small.clone()
        b[3], b[4], b[31] = -0.0, -0.0, -0.0
    elif i == 4:    # scaled maximum in (6, 8): clips to 6
        b = small.clone()
        b[7], b[20] = 7.5, -6.5
    elif i == 5:    # ... at another exponent
        b = small * 32
        b[0] = -7.25 * 32
    elif i == 6:    # a maximum of exactly 4 x 2^-3
        b = small.clamp(-0.4, 0.4)
        b[9] = 0.5
    elif i == 7:    # a maximum of exactly 6 x 2^4
        b = small * 16
        b[30] = -96.0
    elif i == 8:    # clamps at e = -64: everything rounds to (signed) zero
        b = small * 2.0 ** -72
        b[1] = 1.5 * 2.0 ** -70
    elif i == 9:    # clamps at e = +64: 2^70 saturates, 3 x 2^64 and 2^63 are on the grid
        b[0], b[1], b[2], b[3] = 2.0 ** 70, -3.0 * 2.0 ** 64, 2.0 ** 63, -(2.0 ** 68)
    else:           # 10, 11: neighbours 2^12 apart
        b = torch.linspace(-1.5, 1.5, BLOCK) * 2.0 ** (6 if i == 10 else -6)
    return b.bfloat16().float()


def edge_blocks(N, K, seed=0):
    """bf16 weights [N, K]: the N_EDGE edge blocks above laid out block after block from the start of the matrix (as many as it has blocks), random
    weights behind them whose magnitudes spread over 2^-12 .. 2^12 from row to row and, on odd rows, by 2^12 between neighbouring blocks."""
    g = torch.Generator().manual_seed(seed)
    nb = K // BLOCK
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.linspace(-12, 12, N).round())[:, None]
    alt = torch.exp2(6.0 * (1 - 2 * (torch.arange(nb) % 2))).repeat_interleave(BLOCK)      # 2^6, 2^-6, 2^6 ...
    w[1::2] *= alt[None, :]
    w = w.bfloat16().float().view(N * nb, BLOCK)
    for i in range(min(N_EDGE, N * nb)):
        w[i] = _edge(i, g)
    return w.view(N, K).bfloat16()
