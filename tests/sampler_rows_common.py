"""The per-request sampler's rule (include/thinkdiff_hip.h, td_sample_rows_bf16) restated with torch on the CPU, and the statistical bars of
tests/test_sampler_gpu.py as one function.  Shared by tests/test_sampler_rows_cpu.py and tests/test_sampler_rows_gpu.py.

  penalise   repetition, then frequency, then presence penalty on the tokens of the prompt set or with a generated count, in fp32 (the precision the
             rule prescribes), every other token float(x);
  law        p = softmax(z / T) in fp64; sort descending (stable); top-k = the first k; top-p = a token is kept iff the mass in front of it is
             < top_p x (top-k mass); min-p = p >= min_p x max p; the kept set is the intersection, renormalised;
  assert_law the bars of tests/test_sampler_gpu.py::test_top_p_sampler_law, verbatim: support, TV < 1.25 x E[TV] + 3e-3 with boundary ties pooled,
             head frequency within 5 sigma + 1e-4, chi-square over 16 rank-ordered equal-mass bins < 50.
"""
import math

import torch


def penalise(x_bf16_row, prompt_ids=(), counts=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
    """z[vocab] in fp32: the penalised logits of one row.  counts: int tensor [vocab] or None."""
    x = x_bf16_row.float().cpu()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    V = x.numel()
    c = torch.zeros(V, dtype=torch.float32) if counts is None else counts.cpu().float()
    seen = c > 0
    if len(prompt_ids):
        ids = torch.tensor([int(t) for t in prompt_ids if 0 <= int(t) < V], dtype=torch.int64)
        seen = seen.clone()
        seen[ids] = True
    rp = torch.tensor(float(repetition_penalty), dtype=torch.float32)
    z = torch.where(seen, torch.where(x > 0, x / rp, x * rp), x)
    z = torch.where(seen, z - torch.tensor(float(frequency_penalty), dtype=torch.float32) * c, z)
    z = torch.where(seen & (c > 0), z - torch.tensor(float(presence_penalty), dtype=torch.float32), z)
    return z


def kept_mask_sorted(sp, top_k=-1, top_p=1.0, min_p=0.0, min_p_first=False):
    """Keep mask over probabilities sorted descending.  min_p_first: the order of newer vLLM (min-p before top-k / top-p, which then work on the
    min-p survivors renormalised) -- the order the engine does NOT implement; it exists so that a test can pin the difference."""
    V = sp.numel()
    keep = torch.ones(V, dtype=torch.bool)
    if min_p_first and min_p > 0:
        keep &= sp >= min_p * sp[0]
    if 0 < top_k < V:
        k_mask = torch.zeros(V, dtype=torch.bool)
        k_mask[:top_k] = True
        keep &= k_mask
    base = torch.where(keep, sp, torch.zeros_like(sp))
    if top_p < 1.0:
        keep &= (torch.cumsum(base, 0) - base) < top_p * base.sum()
    if not min_p_first and min_p > 0:
        keep &= sp >= min_p * sp[0]
    return keep


def law(z_row, temperature, top_k=-1, top_p=1.0, min_p=0.0, min_p_first=False):
    """-> (q [vocab] fp64: the law of the draw, p_edge: the smallest kept probability, p [vocab]: softmax(z / T))."""
    p = torch.softmax(z_row.double().cpu() / temperature, dim=-1)
    sp, idx = torch.sort(p, descending=True, stable=True)
    keep = kept_mask_sorted(sp, top_k, top_p, min_p, min_p_first)
    kept = torch.where(keep, sp, torch.zeros_like(sp))
    q = torch.zeros_like(p)
    q[idx] = kept / kept.sum()
    return q, float(sp[keep].min()), p


def tv_noise(q, N):
    """E[TV] of N draws from q: 1/2 sum_i sqrt(2 q_i (1 - q_i) / (pi N))."""
    return float(0.5 * (2 * q * (1 - q) / (math.pi * N)).sqrt().sum())


def check_case(q, p, p_edge, N, min_kept=2, min_p=0.0):
    """What a case must satisfy before a GPU result is judged against it: the kept set is what the case intends (at least min_kept tokens), E[TV]
    is finite, and -- the kernel's min-p threshold is an fp32 logit, the restatement's an fp64 probability -- no token sits within 1e-5 (relative) of
    the min-p threshold unless it is the maximum itself."""
    assert int((q > 0).sum()) >= min_kept, f"the case keeps {int((q > 0).sum())} token(s), fewer than intended"
    assert math.isfinite(tv_noise(q, N))
    if 0 < min_p < 1:
        thr = min_p * float(p.max())
        assert not bool(((p / thr - 1).abs() < 1e-5).any()), "a token sits on the min-p threshold: pick another seed"


def assert_law(draws, q, p_full, p_edge, label=""):
    """The bars of tests/test_sampler_gpu.py on int draws [N] against the law q."""
    vocab = q.numel()
    N = draws.numel()
    assert int(draws.min()) >= 0 and int(draws.max()) < vocab
    counts = torch.bincount(draws.cpu().long(), minlength=vocab).double()
    # support: sampled tokens are in the kept set, or tie with its boundary probability
    outside = (counts > 0) & (q == 0)
    assert bool(((p_full[outside] - p_edge).abs() <= 1e-12 * p_edge).all()), f"{label}: a token outside the kept set was sampled"
    # law: tied boundary tokens are interchangeable, so compare after pooling all tokens whose probability equals the edge value
    tie = (p_full - p_edge).abs() <= 1e-12 * p_edge
    emp = counts / counts.sum()
    tv = 0.5 * ((emp[~tie] - q[~tie]).abs().sum() + abs(float(emp[tie].sum() - q[tie].sum())))
    top = int(q.argmax())
    sigma = float((q[top] * (1 - q[top]) / N).sqrt())
    noise = tv_noise(q, N)
    print(f"{label}: kept {int((q > 0).sum())} tokens, TV {float(tv):.4f} (noise {noise:.4f}), head freq {float(emp[top]):.4f} vs {float(q[top]):.4f}")
    assert float(tv) < 1.25 * noise + 3e-3, f"{label}: TV {float(tv):.4f} vs {noise:.4f} expected from sampling noise"
    assert abs(float(emp[top] - q[top])) < 5 * sigma + 1e-4, label
    # systematic bias (a wrong boundary, a skewed draw) shows in coarse bins: 16 rank-ordered bins of equal mass
    order = torch.argsort(q, descending=True)
    cum = torch.cumsum(q[order], 0)
    bin_of = torch.clamp((cum * 16).floor().long(), max=15)
    exp_b = torch.zeros(16, dtype=torch.float64).index_add_(0, bin_of, q[order]) * counts.sum()
    # tokens outside the law's support are boundary ties, interchangeable with the tied tokens inside it: they count in the last bin
    inside = counts[order] * (q[order] > 0)
    obs_b = torch.zeros(16, dtype=torch.float64).index_add_(0, bin_of, inside)
    obs_b[bin_of[int((q[order] > 0).sum()) - 1]] += counts[q == 0].sum()
    ok = exp_b > 0
    chi2 = float((((obs_b - exp_b) ** 2)[ok] / exp_b[ok]).sum())
    print(f"   chi2 over {int(ok.sum())} equal-mass bins {chi2:.1f}")
    assert chi2 < 50.0, f"{label}: chi2 {chi2:.1f}"                 # 15 degrees of freedom: P(chi2 > 50) ~ 1e-5
