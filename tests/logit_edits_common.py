"""The logit-edit rule of td_sample_rows_edit_bf16 (include/thinkdiff_hip.h) restated with torch on the CPU in fp32 / fp64, the brute-force restatement of
vLLM's bad-words and min-tokens rules the ban planner is checked against, and the fp64 logprobs.  Shared by tests/test_logit_edits_cpu.py,
tests/test_logit_edits_gpu.py and tests/test_logprobs_rows_gpu.py; the penalties, the law and its bars are tests/sampler_rows_common.py's.

  edit       z[t] = -inf if t is banned; float(x[t]) + b[t] (one fp32 addition) if t has a bias; float(x[t]) otherwise (NaN -> -inf);
  edited     edit, then sampler_rows_common.penalise on the fp32 z (the repetition sign test sees the biased value);
  banned_at  the set of tokens vLLM's rules ban for a request whose output so far is `output`: everything outside allowed_token_ids, every one-token
             bad word, the last token of a longer bad word iff the output ends with the word's prefix, and -- while fewer than min_tokens tokens
             exist -- EOS (unless ignore_eos) and the stop ids;
  logprobs64 log_softmax in fp64, the stable descending order and vLLM's rank (the number of logits >= the chosen one).
"""
import torch

from sampler_rows_common import penalise, law, check_case, assert_law  # noqa: F401  (re-exported for the tests)


def edit(x_bf16_row, banned=(), bias=None):
    """z[vocab] in fp32: the edited logits of one row.  banned: token ids; bias: dict token -> value."""
    x = x_bf16_row.float().cpu()
    z = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x).clone()
    for t, b in (bias or {}).items():
        v = z[int(t)] + torch.tensor(0.0 if b != b else float(b), dtype=torch.float32)
        z[int(t)] = float("-inf") if bool(torch.isnan(v)) else v
    if len(banned):
        z[torch.tensor([int(t) for t in banned], dtype=torch.int64)] = float("-inf")
    return z


def edited(x_bf16_row, banned=(), bias=None, **penalties):
    return penalise(edit(x_bf16_row, banned, bias), **penalties)      # (penalise takes `.float()` of its row: an fp32 z passes through unchanged)


def banned_at(output, vocab, allowed=None, bad_words=(), stop_ids=(), min_tokens=0, eos=None, ignore_eos=True):
    """Brute force: every rule evaluated from scratch on the whole output."""
    out = set()
    if allowed is not None:
        out |= set(range(vocab)) - {int(t) for t in allowed}
    for w in bad_words:
        w = [int(t) for t in w]
        if len(w) == 1:
            out.add(w[0])
        elif len(w) - 1 <= len(output) and list(output[len(output) - (len(w) - 1):]) == w[:-1]:
            out.add(w[-1])
    if len(output) < min_tokens:
        out |= {int(t) for t in stop_ids if 0 <= int(t) < vocab}
        if not ignore_eos and eos is not None:
            out.add(int(eos))
    return out


def logprobs64(x_bf16_row):
    """-> (lp fp64 [vocab], order: the stable descending order of the logits)."""
    x = x_bf16_row.double().cpu()
    return torch.log_softmax(x, dim=-1), torch.sort(x, descending=True, stable=True).indices


# |lp - lp64| for |lp| <= 64, derived (not tuned): the fp32 ulp below 64 is 3.8e-6, the truncation of a 2^-40 fixed-point sum is below
# V x 2^-40 = 1.4e-7 at V = 152 064, exp2 / log2 are 1-ulp operations
LOGPROB_BAR = 2e-5
