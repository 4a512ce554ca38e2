"""Shared by the per-request LoRA tests (test_qwen2_lora_cpu.py, test_lora_rows_gpu.py, test_qwen2_lora_gpu.py): the float64 restatement of the
row-indexed low-rank add, its error bound, the cases both the CPU and the GPU test run, a synthetic peft-layout adapter and the float64 merge.

**Parity unpinned**: restated from the published peft source (`LoraLayer.forward`: `result + lora_B(lora_A(x)) * scaling`, `scaling = lora_alpha / r`, or
`lora_alpha / sqrt(r)` under `use_rslora`) and peft's `save_pretrained` key layout (`base_model.model.<module>.lora_A.weight` / `.lora_B.weight`); the
definition under test is the one at the top of csrc/lora_rows.hip:

    t_j = bf16_rne( sum_k x_k A_jk )                                 fp32 accumulation, any order
    y_n = bf16_rne( float(y_base_n) + s * sum_j float(t_j) B_nj )    fp32 accumulation; ONE rounding
"""
import torch

MODULES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


# ---- the definition in float64 ------------------------------------------------------------------------------------------------------------------------

def bf16_rne64(v):
    """float64 -> the nearest bf16 value (ties to even), as float64, with no detour through float32 (normal range only)."""
    v = v.double()
    m, e = torch.frexp(v)                                  # v = m 2^e, 0.5 <= |m| < 1: 8 significant bits = m 2^8 rounded
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)  # (torch.round: half to even)


def ulp_bf16(v):
    """Spacing of bf16 values at |v| (float64), 2^(floor(log2 |v|) - 7); the smallest normal's for 0."""
    a = v.double().abs().clamp_min(2.0 ** -126)
    return torch.ldexp(torch.ones_like(a), (torch.floor(torch.log2(a)) - 7).to(torch.int32))


def pad16(r):
    return (r + 15) // 16 * 16


def segment_ref(x, y_base, row_adapter, pairs, scales):
    """One output segment by the definition, in float64.  x bf16 [rows, K]; y_base bf16 [rows, N]; row_adapter ints [rows]; pairs[a] = (A [r, K], B [N, r])
    bf16 or None; scales[a].  Returns (y float64 holding bf16 values, touched bool [rows], t float64 [rows, r_max])."""
    rows = x.shape[0]
    y = y_base.double().clone()
    touched = torch.zeros(rows, dtype=torch.bool)
    ts = {}
    for a, pair in enumerate(pairs):
        if pair is None:
            continue
        sel = torch.tensor([int(v) == a for v in row_adapter])
        if not bool(sel.any()):
            continue
        A, B = pair
        t = bf16_rne64(x[sel].double() @ A.double().T)
        y[sel] = bf16_rne64(y_base[sel].double() + float(scales[a]) * (t @ B.double().T))
        touched |= sel
        ts[a] = t
    return y, touched, ts


def segment_bound(x, y_base, row_adapter, pairs, scales):
    """Per output element, how far a kernel that follows the definition in fp32 -- in any summation order -- may land from segment_ref.

    The kernel computes t'_j = bf16(S'_j), S'_j an fp32 sum of exact products in some order, so |S'_j - S_j| <= K 2^-24 sum_k |x_k A_jk| =: e_j (the
    standard bound for K - 1 fp32 additions, u = 2^-24, first order).  Rounding S'_j instead of S_j moves t_j by at most e_j and, where that crosses a
    rounding boundary, by one more bf16 spacing: |t'_j - t_j| <= ulp_bf16(t_j) + e_j.  Through the second product that is
        |s| sum_j |B_nj| ulp_bf16(t_j)   +   |s| sum_j |B_nj| e_j.
    The second sum has r_pad terms and joins s and y_base in fp32: (r_pad + 2) 2^-24 (|y_base| + |s| sum_j |t_j B_nj|).  Both results are then rounded to
    bf16 once; two numbers this close round to values at most the distance plus one bf16 spacing of the reference apart."""
    K = x.shape[1]
    bound = torch.zeros(y_base.shape, dtype=torch.float64)
    y_ref, _, ts = segment_ref(x, y_base, row_adapter, pairs, scales)
    for a, t in ts.items():
        A, B = pairs[a]
        s = abs(float(scales[a]))
        sel = torch.tensor([int(v) == a for v in row_adapter])
        e = K * 2.0 ** -24 * (x[sel].double().abs() @ A.double().abs().T)                       # [rows_a, r]
        Babs = B.double().abs().T                                                               # [r, N]
        term1 = s * (ulp_bf16(t) @ Babs)
        term2 = s * (e @ Babs)
        term3 = (pad16(A.shape[0]) + 2) * 2.0 ** -24 * (y_base[sel].double().abs() + s * (t.abs() @ Babs))
        bound[sel] = ulp_bf16(y_ref[sel]) + term1 + term2 + term3
    return bound


def segment_f32(x, y_base, row_adapter, pairs, scales, chunk=96):
    """A float32 restatement of the kernel in ANOTHER summation order (K in chunks of `chunk`, added last to first): it must meet segment_bound, or the
    bound is wrong."""
    y = y_base.clone()
    for a, pair in enumerate(pairs):
        if pair is None:
            continue
        sel = torch.tensor([int(v) == a for v in row_adapter])
        if not bool(sel.any()):
            continue
        A, B = pair
        xs = x[sel].float()
        acc = torch.zeros(xs.shape[0], A.shape[0])
        for k0 in reversed(range(0, x.shape[1], chunk)):
            acc = acc + xs[:, k0:k0 + chunk] @ A.float()[:, k0:k0 + chunk].T
        t = acc.bfloat16().float()
        u = torch.zeros(xs.shape[0], B.shape[0])
        for j in reversed(range(A.shape[0])):
            u = u + t[:, j:j + 1] * B.float()[:, j][None, :]
        y[sel] = (y_base[sel].float() + torch.tensor(float(scales[a]), dtype=torch.float32) * u).bfloat16()
    return y


# ---- the cases of the kernel tests ---------------------------------------------------------------------------------------------------------------------

# name -> (buffers: [columns of buffer b], segments: [(buffer, first column, width)])
LAYOUTS = {
    "one": ([512], [(0, 0, 512)]),                                         # o_proj / down_proj
    "two": ([2048], [(0, 0, 1024), (0, 1024, 1024)]),                      # gate | up in one buffer
    "three": ([512 + 24, 512 + 40], [(0, 0, 512), (1, 0, 256), (1, 256, 256)]),   # q | k | v: q into one buffer, k | v into another, padded leading dimensions
}
ROWS = (1, 3, 16, 17, 33)
RANKS = (1, 5, 16, 64)
KS = (512, 1536)
K_SPLIT = 8960          # run once, at 3 rows: K split over 32 slabs
SENTINEL = 77.0         # the padding columns of a buffer hold this


def mixed_assignment(rows, n_adapters, g):
    """Adapters interleaved inside 16-row tiles with -1 rows among them."""
    v = torch.randint(-1, n_adapters, (rows,), generator=g).tolist()
    if rows >= 3:
        v[0], v[1], v[2] = 0, -1, n_adapters - 1
    elif all(a < 0 for a in v):
        v[0] = 0
    return v


def make_case(layout, rows, K, ranks, seed, exact=False, null=(), assignment=None, zero_B=()):
    """x, the output buffers with their base values, the row -> adapter assignment and one pair per (adapter, segment).
    exact: x, A, B in {-1, 0, 1} with at most 200 non-zeros per x row (every t_j an integer of magnitude <= 200 <= 256), y_base small integers, scales in
    {0.5, 2}: every sum is exact in fp32 in any order.  null: (adapter, segment) places without a pair; zero_B: adapters whose B is all zero."""
    g = torch.Generator().manual_seed(seed)
    cols, segs = LAYOUTS[layout]
    n_ad = len(ranks)
    if exact:
        x = torch.zeros(rows, K)
        for r in range(rows):
            idx = torch.randperm(K, generator=g)[:200]
            x[r, idx] = torch.randint(0, 2, (200,), generator=g).float() * 2 - 1
        bufs = [torch.randint(-8, 9, (rows, c), generator=g).float() for c in cols]
        scales = [(0.5, 2.0)[a % 2] for a in range(n_ad)]
    else:
        x = torch.randn(rows, K, generator=g)
        bufs = [torch.randn(rows, c, generator=g) for c in cols]
        scales = [2.0 if a % 2 == 0 else 2.0 * r / r ** 0.5 for a, r in enumerate(ranks)]      # lora_alpha = 2 r, plain and under use_rslora
    for b, c in enumerate(cols):       # sentinel columns past the segments of the buffer
        used = max(c0 + w for (bb, c0, w) in segs if bb == b)
        bufs[b][:, used:] = SENTINEL
    pairs = []
    for a, r in enumerate(ranks):
        per = []
        for s, (_, _, w) in enumerate(segs):
            if exact:
                A = torch.randint(-1, 2, (r, K), generator=g).float()
                B = torch.randint(-1, 2, (w, r), generator=g).float()
            else:
                A = 0.05 * torch.randn(r, K, generator=g)
                B = 0.05 * torch.randn(w, r, generator=g)
            if a in zero_B:
                B = torch.zeros(w, r)
            per.append(None if (a, s) in null else (A.bfloat16(), B.bfloat16()))
        pairs.append(per)
    if assignment is None:
        assignment = mixed_assignment(rows, n_ad, g)
    return {"layout": layout, "x": x.bfloat16(), "bufs": [b.bfloat16() for b in bufs], "segs": segs, "row_adapter": assignment, "pairs": pairs, "ranks": list(ranks),
            "scales": scales}


def case_views(case, bufs):
    """The output segments as views of `bufs`."""
    return [bufs[b][:, c0:c0 + w] for (b, c0, w) in case["segs"]]


def case_ref(case):
    """Per segment (y float64, touched rows, bound) by the definition."""
    out = []
    for s, base in enumerate(case_views(case, case["bufs"])):
        per = [p[s] for p in case["pairs"]]
        y, touched, _ = segment_ref(case["x"], base, case["row_adapter"], per, case["scales"])
        out.append((y, touched, segment_bound(case["x"], base, case["row_adapter"], per, case["scales"])))
    return out


def random_cases():
    """The random-operand cases of the kernel tests: four adapters of ranks (5, 16, 64, 16), adapter 1 without a pair for the first segment."""
    for li, layout in enumerate(LAYOUTS):
        for rows in ROWS:
            for K in KS:
                yield make_case(layout, rows, K, (5, 16, 64, 16), seed=1000 + 100 * li + rows + K, null={(1, 0)})
    yield make_case("three", 3, K_SPLIT, (5, 16, 64, 16), seed=1999, null={(1, 0)}, assignment=[0, 2, 3])


# ---- adapters on the decoder ---------------------------------------------------------------------------------------------------------------------------

def module_shapes(cfg):
    """{module: (N, K)} of the 7 Linears of a decoder layer."""
    D, I, QW, HW = cfg.hidden, cfg.intermediate, cfg.num_heads * 128, cfg.num_kv_heads * 128
    return {"self_attn.q_proj": (QW, D), "self_attn.k_proj": (HW, D), "self_attn.v_proj": (HW, D), "self_attn.o_proj": (D, QW), "mlp.gate_proj": (I, D),
            "mlp.up_proj": (I, D), "mlp.down_proj": (D, I)}


def make_adapter(cfg, rank, seed, modules=MODULES, std=0.05, prefix="base_model.model.", use_rslora=False, b_std=None):
    """A synthetic adapter in peft's published layout: (state dict, adapter_config dict).  A ~ std N(0, 1), B ~ b_std N(0, 1) (default: std) rounded to bf16,
    lora_alpha = 2 r."""
    b_std = std if b_std is None else b_std
    g = torch.Generator().manual_seed(seed)
    shapes = module_shapes(cfg)
    sd = {}
    for i in range(cfg.num_layers):
        for m in modules:
            N, K = shapes[m]
            sd[f"{prefix}model.layers.{i}.{m}.lora_A.weight"] = (std * torch.randn(rank, K, generator=g)).bfloat16()
            sd[f"{prefix}model.layers.{i}.{m}.lora_B.weight"] = (b_std * torch.randn(N, rank, generator=g)).bfloat16()
    config = {"peft_type": "LORA", "r": rank, "lora_alpha": 2 * rank, "use_rslora": use_rslora, "use_dora": False, "bias": "none", "modules_to_save": None,
              "rank_pattern": {}, "alpha_pattern": {}, "target_modules": sorted({m.split(".")[-1] for m in modules})}
    return sd, config


def adapter_scale(config):
    r = config["r"]
    return config["lora_alpha"] / (r ** 0.5 if config.get("use_rslora") else r)


def merged_state_dict(sd, adapter_sd, config, dtype=torch.float32, prefix="base_model.model."):
    """W' = W + s B A in float64, rounded once to `dtype`; untouched tensors are cast to `dtype`."""
    s = adapter_scale(config)
    out = {}
    for k, v in sd.items():
        a = adapter_sd.get(f"{prefix}{k[:-len('.weight')]}.lora_A.weight") if k.endswith(".weight") else None
        if a is not None:
            b = adapter_sd[f"{prefix}{k[:-len('.weight')]}.lora_B.weight"]
            v = v.double() + s * (b.double() @ a.double())
        out[k] = v.to(dtype)
    return out


def rel_rmse(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
