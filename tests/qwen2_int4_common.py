"""CPU restatement of the grouped int4 weight format of the Qwen2-VL decode engine (include/thinkdiff_hip.h, "grouped int4 weight stream"), shared by
tests/test_qwen2_int4_cpu.py and tests/test_qwen2_int4_gpu.py.

Format: asymmetric uint4 under one fp16 scale and one 4-bit zero point per group of G consecutive k of a row of W[N, K]:
  q, z in 0 .. 15, s a finite fp16;   W^ = bf16_rne(fp32(q - z) * fp32(s)) -- the product is exact in fp32 (5 x 11 significant bits), so ONE rounding.
The two checkpoint layouts are packed and unpacked here from their definitions (AutoAWQ "GEMM", AutoGPTQ 4-bit), with plain torch integer arithmetic;
nothing in here, and no test, knows the order of the nibbles inside the library's own `packed` bytes: those are reached through td_repack_int4 only.
All functions take and return (q uint8 [N, K], z uint8 [N, K / G], s float16 [N, K / G]) in the Linear's own orientation (row n = output feature n).
"""
import torch

from qwen2_w8_common import linear_tol, sum_bound, ulp_bf16  # noqa: F401  (the analytic bound is the same bound: exact products, fp32 sum in some order)

AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)      # nibble p of an AutoAWQ int32 holds element AWQ_ORDER[p] of its 8
LAYOUT_AWQ, LAYOUT_GPTQ, LAYOUT_GPTQ_V2 = 0, 1, 3      # td_repack_int4's layout argument (GPTQ_V2 = GPTQ | the v2 flag)


def w_hat(q, z, s, G):
    """-> W^ bf16 [N, K]: ((q - z).float() * s.float()).bfloat16().  (Where q == z under a negative scale this zero is -0 and the library's is +0: the
    tests compare values, to which the sign of a zero weight is nothing.)"""
    zz = z.to(torch.int32).repeat_interleave(G, dim=1)
    ss = s.float().repeat_interleave(G, dim=1)
    return ((q.to(torch.int32) - zz).float() * ss).bfloat16()


def _pack_nibbles(v, order):
    """v int64 [..., 8 m] with values 0 .. 15 -> int32 [..., m]: nibble p of word j holds v[..., 8 j + order[p]]."""
    v = v.reshape(*v.shape[:-1], v.shape[-1] // 8, 8).to(torch.int64)
    word = torch.zeros(v.shape[:-1], dtype=torch.int64, device=v.device)
    for p, e in enumerate(order):
        word |= (v[..., e] & 15) << (4 * p)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)      # the same 32 bits as a signed word


def _unpack_nibbles(word, order):
    """int32 [..., m] -> int64 [..., 8 m], the inverse of _pack_nibbles."""
    w = word.to(torch.int64) & 0xFFFFFFFF
    out = torch.empty(*word.shape, 8, dtype=torch.int64, device=word.device)
    for p, e in enumerate(order):
        out[..., e] = (w >> (4 * p)) & 15
    return out.reshape(*word.shape[:-1], word.shape[-1] * 8)


def pack_awq(q, z, s):
    """-> {"qweight": int32 [K, N / 8], "qzeros": int32 [K / G, N / 8], "scales": fp16 [K / G, N]}: AutoAWQ "GEMM" (w = x @ qweight-as-[K, N])."""
    return {"qweight": _pack_nibbles(q.T.contiguous(), AWQ_ORDER), "qzeros": _pack_nibbles(z.T.contiguous(), AWQ_ORDER), "scales": s.T.contiguous()}


def unpack_awq(t):
    q = _unpack_nibbles(t["qweight"], AWQ_ORDER).T.contiguous().to(torch.uint8)
    z = _unpack_nibbles(t["qzeros"], AWQ_ORDER).T.contiguous().to(torch.uint8)
    return q, z, t["scales"].T.contiguous()


def pack_gptq(q, z, s, v2=False, g_idx=True):
    """-> {"qweight": int32 [K / 8, N] (nibble p of row r = q[8 r + p, n]), "qzeros": int32 [K / G, N / 8] (nibble p of column c = z[g, 8 c + p] - 1, or z itself
    with v2), "scales": fp16 [K / G, N], "g_idx": int32 [K] = k // G}: AutoGPTQ, 4 bits, no act-order."""
    N, K = q.shape
    G = K // z.shape[1]
    qw = _pack_nibbles(q.contiguous(), range(8)).T.contiguous()                       # along k, then [K / 8, N]
    stored = z.to(torch.int64) if v2 else (z.to(torch.int64) - 1) & 15
    out = {"qweight": qw, "qzeros": _pack_nibbles(stored.T.contiguous(), range(8)), "scales": s.T.contiguous()}
    if g_idx:
        out["g_idx"] = (torch.arange(K) // G).to(torch.int32)
    return out


def unpack_gptq(t, v2=False):
    q = _unpack_nibbles(t["qweight"].T.contiguous(), range(8)).to(torch.uint8)
    stored = _unpack_nibbles(t["qzeros"], range(8)).T.contiguous()
    z = (stored if v2 else (stored + 1) & 15).to(torch.uint8)
    return q, z, t["scales"].T.contiguous()


def pack(layout, q, z, s):
    return pack_awq(q, z, s) if layout == LAYOUT_AWQ else pack_gptq(q, z, s, v2=layout == LAYOUT_GPTQ_V2)


EDGE_SCALES = (2.0 ** -24, 65504.0, -65504.0, -1.0, 0.5, 2.0, 1023 * 2.0 ** -24, -0.0072021484375, 3 * 2.0 ** -24, 2.0 ** -14, 1.0, 0.333251953125, 1000.0, -3.0e-5)


def edge_problem(N, K, G, seed=0):
    """(q, z, s) whose rows run through all 256 (q, z) pairs group after group, under scales that include fp16 subnormals, the largest fp16, negative
    values and powers of two (EDGE_SCALES), then random fp16 scales of every magnitude."""
    g = torch.Generator().manual_seed(seed)
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    grp = k // G
    z = ((torch.arange(K // G)[None, :] + 5 * n) % 16).to(torch.uint8)
    q = ((k % G + 7 * grp + 3 * n) % 16).to(torch.uint8)               # G >= 32 consecutive k: every q meets the group's z
    s = (torch.randn(N, K // G, generator=g) * torch.exp2(torch.randint(-20, 12, (N, K // G), generator=g).float())).half()
    s[~torch.isfinite(s)] = 1.0
    edge = torch.tensor(EDGE_SCALES, dtype=torch.float32).half()
    flat = s.view(-1)
    flat[:min(len(edge), flat.numel())] = edge[:flat.numel()]
    return q, z, s


def random_problem(N, K, G, seed=0, device="cpu"):
    """Uniform random nibbles and zero points under scales of magnitude 2^-9 .. 2^-6, either sign (made where they are used)."""
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.randint(0, 16, (N, K), generator=g, device=device, dtype=torch.uint8)
    z = torch.randint(0, 16, (N, K // G), generator=g, device=device, dtype=torch.uint8)
    s = ((torch.rand(N, K // G, generator=g, device=device) + 1.0) * 2.0 ** -9 * torch.exp2(torch.randint(0, 3, (N, K // G), generator=g, device=device).float()))
    sign = torch.randint(0, 2, (N, K // G), generator=g, device=device).float() * 2 - 1
    return q, z, (s * sign).half()


def bf16_bits(t):
    return t.to(torch.bfloat16).contiguous().view(torch.int16)


LINEAR_KEYS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def int4_state_dict(sd, layout, G, seed=0):
    """A bf16 state dict -> (the checkpoint-style dict in which every decoder Linear is `<linear>.qweight / .qzeros / .scales` (+ `.g_idx` for GPTQ) with
    random nibbles under scales of the weight's own magnitude, the same dict with those Linears as the restatement's W^ in bf16).  Not a quantiser: the
    nibbles do not approximate the bf16 weights, they replace them (the engine has no int4 quantiser either)."""
    ck, hat = {}, {}
    for i, (k, v) in enumerate(sd.items()):
        base, _, suffix = k.rpartition(".")
        if suffix == "weight" and base.split(".")[-1] in LINEAR_KEYS:
            N, K = v.shape
            q, z, _ = random_problem(N, K, G, seed=seed + i)
            g = torch.Generator().manual_seed(seed + 7919 * i)
            s = ((torch.rand(N, K // G, generator=g) + 0.5) * float(v.float().std()) / 6.0).half()
            for name, t in pack(layout, q, z, s).items():
                ck[base + "." + name] = t
            hat[k] = w_hat(q, z, s, G).to(v.dtype)
        else:
            ck[k] = hat[k] = v
    return ck, hat
