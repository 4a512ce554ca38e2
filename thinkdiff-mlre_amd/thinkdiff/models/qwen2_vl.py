"""Qwen2-VL text decoder on the HIP engine (`td_qwen2_*`): hidden states at `model.norm` and sampling.

Stands in for the `vllm.LLM(model="Qwen/Qwen2-VL-*", return_hidden_states=True)` object of the reference
(thinkdiff/models/mllama_vllm_t5_embed_decoder_2.py:790-816; thinkdiff/models/mllama_vllm_generate_1.py:382-413)
for the part of its behaviour the ThinkDiff path uses: `generate()` returning, per request, the prompt tokens'
and the generated tokens' hidden states at `embedding_layer_name="model.norm"` plus the generated token ids.
Image inputs: `vision_towers.HipQwen2VisionTransformer` produces the merged vision tokens; `expand_image_placeholders`,
`embed_tokens` and `mrope_position_ids` below do what vLLM's input processor and `get_rope_index` do around the decoder.
"""
import collections
import ctypes
import dataclasses
import numbers
from collections import deque
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _hip
from ..ops import register as _register_ops
from . import prefix_cache as _pfx
from . import qwen2_lora as _lora
from .qwen2_lora import LoRARequest      # noqa: F401  (vLLM's name, importable from here as SamplingParams is)
_OPS = _register_ops()      # torch.ops.thinkdiff_hip: the custom-op layer over the C ABI (GPU kernels only, no fallback)
_KEEP = object()            # forward(lora_request=...): leave the slot's adapter as it is


def _prefix_entry(fn):
    """A generate entry under automatic prefix caching: while it runs, the low-level writers it calls (forward, fork_slot, gather_slots, ..) do not drop the
    cache's entries -- the entry keeps the books itself -- and whatever it leaves live is retained when it returns or raises.  With the feature off: fn."""
    import functools

    @functools.wraps(fn)
    def run(self, *a, **kw):
        if getattr(self, "_lora", None) is None:
            return cached(self, *a, **kw)
        self._lora_depth = getattr(self, "_lora_depth", 0) + 1
        try:
            return cached(self, *a, **kw)
        finally:      # per-request LoRA: when the outermost entry returns or raises, no cache slot names an adapter any more
            self._lora_depth -= 1
            if self._lora_depth == 0:
                self._lora.release_all()

    def cached(self, *a, **kw):
        pc = getattr(self, "_prefix_cache", None)
        if pc is None:
            return fn(self, *a, **kw)
        self._pc_depth = getattr(self, "_pc_depth", 0) + 1
        if self._pc_depth == 1:
            pc.release_all()
        try:
            return fn(self, *a, **kw)
        finally:
            self._pc_depth -= 1
            if self._pc_depth == 0:
                pc.release_all()
    return run


class _CacheSlots:
    """The free-slot stack of generate_batch / generate_continuous while prefix caching is on: slots come from the cache's allocator (free ones first,
    then retained ones, least recently used first) and a finished sequence's slot goes back retained."""

    def __init__(self, pc):
        self.pc = pc

    def pop(self):
        s = self.pc.take(1)
        if s is None:
            raise _hip.ThinkDiffHipError("prefix cache: no cache slot left for a new sequence")
        return s[0]

    def extend(self, slots):
        for s in slots:
            self.pc.release(int(s))

    def __getitem__(self, i):      # ([-1]: a slot to run a prompt-only forward through -- it holds nothing afterwards)
        s = self.pop()
        self.pc.drop(s)
        return s


@dataclasses.dataclass
class Qwen2VLTextConfig:
    """Text-side keys of [ext] Qwen/Qwen2-VL-7B-Instruct config.json (2B: 1536 / 12 / 2 / 8960 / 151936 / tied)."""
    hidden_size: int = 3584
    num_hidden_layers: int = 28
    num_attention_heads: int = 28
    num_key_value_heads: int = 4
    intermediate_size: int = 18944
    vocab_size: int = 152064
    tie_word_embeddings: bool = False
    mrope_section: Sequence[int] = (16, 24, 24)
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1e6


@dataclasses.dataclass
class SamplingParams:
    """The fields of vllm.SamplingParams the reference sets (mllama_vllm_t5_embed_decoder_2.py:817-823), and the ones a user sets next: top_k, min_p,
    the three penalties and a per-request seed, under vLLM's names, defaults and ranges.  With every one of those at its default the engine samples
    with td_sample_top_p_bf16 as before; any other value routes the call through the per-request sampler (td_sample_rows_bf16)."""
    temperature: float = 0.6
    top_p: float = 0.9
    max_tokens: int = 128
    min_tokens: int = 128
    ignore_eos: bool = True
    stop_token_ids: Optional[List[int]] = None
    top_k: int = -1
    min_p: float = 0.0
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    seed: Optional[int] = None
    # logit edits (td_sample_rows_edit_bf16: applied in front of the penalties, in vLLM's order) and logprobs (td_logprobs_rows_bf16, raw logits)
    logit_bias: Optional[Dict[int, float]] = None
    allowed_token_ids: Optional[List[int]] = None
    bad_words_token_ids: Optional[List[List[int]]] = None      # vLLM's bad words, already tokenised (string `bad_words` need a tokenizer: not served)
    mask_stop_below_min_tokens: bool = False      # True: vLLM's min_tokens rule (EOS and the stop ids cannot be sampled before min_tokens); False: they are sampled and only do not stop
    logprobs: Optional[int] = None
    # parallel sampling: the request is prefilled once and runs as k = best_of or n sequences on forked cache slots (td_qwen2_fork_slot); n of them are
    # returned, the most probable n by cumulative logprob when best_of > n
    n: int = 1
    best_of: Optional[int] = None

    def validate(self) -> "SamplingParams":
        """vLLM's ranges; a ValueError names the field and the value."""
        def bad(field, why):
            raise ValueError(f"SamplingParams.{field}={getattr(self, field)!r}: {why}")

        def token(t):
            return isinstance(t, numbers.Integral) and not isinstance(t, bool) and t >= 0
        if self.logit_bias is not None:
            if not hasattr(self.logit_bias, "items"):
                bad("logit_bias", "must be a dict token id -> bias, or None")
            if len(self.logit_bias) > _hip.MAX_LOGIT_BIAS:
                bad("logit_bias", f"holds {len(self.logit_bias)} entries, at most {_hip.MAX_LOGIT_BIAS} are served")
            for t, v in self.logit_bias.items():
                if not token(t):
                    bad("logit_bias", f"token id {t!r} must be an integer >= 0")
                if isinstance(v, bool) or not isinstance(v, numbers.Real) or v != v or v in (float("inf"), float("-inf")):
                    bad("logit_bias", f"the bias of token {t} must be a finite number, got {v!r}")
        if self.allowed_token_ids is not None:
            if isinstance(self.allowed_token_ids, (str, bytes)) or not hasattr(self.allowed_token_ids, "__len__") or len(self.allowed_token_ids) == 0:
                bad("allowed_token_ids", "must be a non-empty list of token ids, or None")
            if not all(token(t) for t in self.allowed_token_ids):
                bad("allowed_token_ids", "every token id must be an integer >= 0")
        if self.bad_words_token_ids is not None:
            if isinstance(self.bad_words_token_ids, (str, bytes)) or not hasattr(self.bad_words_token_ids, "__len__"):
                bad("bad_words_token_ids", "must be a list of token-id lists, or None")
            for w in self.bad_words_token_ids:
                if isinstance(w, (str, bytes)) or not hasattr(w, "__len__") or len(w) == 0 or not all(token(t) for t in w):
                    bad("bad_words_token_ids", f"every word must be a non-empty list of token ids >= 0, got {w!r}")
        if not (isinstance(self.n, numbers.Integral) and not isinstance(self.n, bool) and self.n >= 1):
            bad("n", "must be an integer >= 1")
        if self.best_of is not None and not (isinstance(self.best_of, numbers.Integral) and not isinstance(self.best_of, bool) and self.best_of >= self.n):
            bad("best_of", f"must be None or an integer >= n={self.n}")
        if not isinstance(self.mask_stop_below_min_tokens, bool):
            bad("mask_stop_below_min_tokens", "must be True or False")
        if self.logprobs is not None and not (isinstance(self.logprobs, numbers.Integral) and not isinstance(self.logprobs, bool)
                                              and 0 <= self.logprobs <= _hip.MAX_LOGPROBS):
            bad("logprobs", f"must be None or an integer in [0, {_hip.MAX_LOGPROBS}]")
        if not (isinstance(self.top_k, numbers.Integral) and not isinstance(self.top_k, bool) and self.top_k >= -1):
            bad("top_k", "must be -1 or 0 (off) or an integer >= 1")
        for f in ("min_p", "top_p", "repetition_penalty", "presence_penalty", "frequency_penalty", "temperature"):
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or v != v or v in (float("inf"), float("-inf")):
                bad(f, "must be a finite number")
        if not 0.0 <= self.min_p <= 1.0:
            bad("min_p", "must be in [0, 1]")
        if not 0.0 < self.top_p <= 1.0:
            bad("top_p", "must be in (0, 1]")
        if not self.repetition_penalty > 0.0:
            bad("repetition_penalty", "must be > 0")
        for f in ("presence_penalty", "frequency_penalty"):
            if not -2.0 <= getattr(self, f) <= 2.0:
                bad(f, "must be in [-2, 2]")
        if self.temperature < 0.0:
            bad("temperature", "must be >= 0")
        if self.seed is not None and (isinstance(self.seed, bool) or not isinstance(self.seed, numbers.Integral)):
            bad("seed", "must be an integer or None")
        if not (isinstance(self.max_tokens, numbers.Integral) and self.max_tokens >= 0):
            bad("max_tokens", "must be an integer >= 0")
        if not (isinstance(self.min_tokens, numbers.Integral) and self.min_tokens >= 0):
            bad("min_tokens", "must be an integer >= 0")
        return self

    @property
    def has_penalty(self) -> bool:
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0

    @property
    def per_request(self) -> bool:
        """True when a field td_sample_top_p_bf16 does not serve is set."""
        return self.top_k > 0 or self.min_p > 0.0 or self.has_penalty or self.seed is not None or self.has_edit or self.width > 1

    @property
    def width(self) -> int:
        """k: the sequences the request runs as (best_of, or n), each on a cache slot of its own."""
        return int(self.n if self.best_of is None else self.best_of)

    def children(self) -> List["SamplingParams"]:
        """The SamplingParams of the k sequences of a request with k > 1 ([self] otherwise).  Child i of a request with seed s draws from
        (s + i, its own token count, 0) -- vLLM V1's child seeds -- and unseeded children draw like any other unseeded live rows.  With best_of > n every
        child is scored (logprobs = 0: the chosen token only) unless the request asked for more."""
        k = self.width
        if k == 1:
            return [self]
        lp = self.logprobs if self.logprobs is not None else (0 if k > self.n else None)
        return [dataclasses.replace(self, n=1, best_of=None, seed=None if self.seed is None else int(self.seed) + i, logprobs=lp) for i in range(k)]

    @property
    def has_edit(self) -> bool:
        """True when the request edits its logits (td_sample_rows_edit_bf16): a bias, an allowed set, bad words, or the min_tokens stop mask with
        something to mask (an EOS id is only known to the generate call: `not ignore_eos` counts as "maybe")."""
        return bool(self.logit_bias) or self.allowed_token_ids is not None or bool(self.bad_words_token_ids) or \
            (self.mask_stop_below_min_tokens and self.min_tokens > 0 and (bool(self.stop_token_ids) or not self.ignore_eos))


SAMPLER_CONFIG_KEYS = ("top_k", "min_p", "repetition_penalty", "presence_penalty", "frequency_penalty", "seed")
LOGIT_EDIT_CONFIG_KEYS = ("logit_bias", "allowed_token_ids", "bad_words_token_ids", "mask_stop_below_min_tokens", "logprobs")
PARALLEL_CONFIG_KEYS = ("n", "best_of")
# vllm.SamplingParams keys the engine does not serve: a vllm_config that sets one is refused, never ignored
UNSERVED_CONFIG_KEYS = {"prompt_logprobs": "prompt_logprobs is not served by the HIP engine (logprobs of generated or forced tokens are: `logprobs`)",
                        "bad_words": "string bad_words need a tokenizer, which the engine does not hold: pass the words as token ids in bad_words_token_ids"}


def lora_engine_kwargs_from_vllm_config(vc) -> dict:
    """vllm_config's enable_lora / max_loras / max_lora_rank as Qwen2VLTextEngine keyword arguments ({} with LoRA off) plus "lora_request" (a LoRARequest or
    None); the keys vLLM has and the engine does not serve are a ValueError naming the key (thinkdiff/models/qwen2_lora.py)."""
    f = _lora.lora_fields_from_vllm_config(vc)
    kw = {"enable_lora": True, "max_loras": f["max_loras"], "max_lora_rank": f["max_lora_rank"]} if f["enable_lora"] else {}
    return {"engine": kw, "lora_request": f["lora_request"]}


def sampler_fields_from_vllm_config(vc) -> dict:
    """The per-request sampler, logit-edit, logprobs and parallel-sampling fields a vllm_config sets, under SamplingParams' names; absent keys (and None) keep the
    defaults.  A key of UNSERVED_CONFIG_KEYS that is set raises a ValueError saying what to use instead."""
    for k, why in UNSERVED_CONFIG_KEYS.items():
        if vc.get(k) is not None:
            raise ValueError(f"vllm_config {k}={vc[k]!r}: {why}")
    return {k: vc[k] for k in SAMPLER_CONFIG_KEYS + LOGIT_EDIT_CONFIG_KEYS + PARALLEL_CONFIG_KEYS if vc.get(k) is not None}


@dataclasses.dataclass
class BeamSearchParams:
    """vllm.sampling_params.BeamSearchParams under vLLM's names (`LLM.beam_search`).  The candidates of a step are RAW logprobs (td_logprobs_rows_bf16), on
    which a temperature could not act: any value but 0 is refused, not ignored."""
    beam_width: int
    max_tokens: int
    ignore_eos: bool = False
    temperature: float = 0.0
    length_penalty: float = 1.0

    def validate(self) -> "BeamSearchParams":
        def bad(field, why):
            raise ValueError(f"BeamSearchParams.{field}={getattr(self, field)!r}: {why}")

        def integer(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, bool)
        if not (integer(self.beam_width) and 1 <= self.beam_width <= _hip.MAX_BEAM_WIDTH):
            bad("beam_width", f"must be an integer in [1, {_hip.MAX_BEAM_WIDTH}] (a step scores 2 x beam_width candidates per beam, at most {_hip.MAX_LOGPROBS})")
        if not (integer(self.max_tokens) and self.max_tokens >= 1):
            bad("max_tokens", "must be an integer >= 1")
        if not isinstance(self.ignore_eos, bool):
            bad("ignore_eos", "must be True or False")
        if isinstance(self.temperature, bool) or not isinstance(self.temperature, numbers.Real) or self.temperature != 0:
            bad("temperature", "beam search ranks raw logprobs, only temperature 0 is served")
        lp = self.length_penalty
        if isinstance(lp, bool) or not isinstance(lp, numbers.Real) or lp != lp or lp in (float("inf"), float("-inf")):
            bad("length_penalty", "must be a finite number")
        return self

    def score(self, cumulative_logprob: float, seq_len: int) -> float:
        """vLLM's get_beam_search_score: cum / seq_len ** length_penalty (seq_len = prompt + generated tokens, less a final EOS)."""
        return float(cumulative_logprob) / (float(seq_len) ** float(self.length_penalty))


BEAM_CONFIG_KEYS = ("beam_width", "length_penalty")


def beam_params_from_vllm_config(vc, max_tokens: int = 128, ignore_eos: bool = False) -> Optional[BeamSearchParams]:
    """The BeamSearchParams a vllm_config asks for with `beam_width` (None without it: generation samples as before).  max_tokens, ignore_eos and
    temperature are the config's own keys where it sets them (a temperature other than 0 beside beam_width is refused by validate()); beam_width
    beside n / best_of > 1 is a ValueError: the two are different ways to spend a request's cache slots."""
    if vc.get("beam_width") is None:
        if vc.get("length_penalty") is not None:
            raise ValueError(f"vllm_config length_penalty={vc['length_penalty']!r} without beam_width: it only acts on a beam search")
        return None
    wide = {k: vc[k] for k in PARALLEL_CONFIG_KEYS if vc.get(k) is not None and vc[k] != 1}
    if wide:
        raise ValueError(f"vllm_config beam_width={vc['beam_width']!r} together with {wide}: beam search returns its beams, n / best_of do not apply")
    return BeamSearchParams(beam_width=vc["beam_width"], max_tokens=vc["max_tokens"] if vc.get("max_tokens") is not None else max_tokens,
                            ignore_eos=vc["ignore_eos"] if vc.get("ignore_eos") is not None else ignore_eos,
                            temperature=vc["temperature"] if vc.get("temperature") is not None else 0.0,
                            length_penalty=vc["length_penalty"] if vc.get("length_penalty") is not None else 1.0).validate()


SPECULATIVE_CONFIG_KEYS = ("method", "num_speculative_tokens", "prompt_lookup_max", "prompt_lookup_min")


@dataclasses.dataclass
class SpeculativeConfig:
    """vLLM's `speculative_config` for the one method served, "ngram" (prompt lookup): up to num_speculative_tokens guessed tokens per sequence and step,
    found by matching the last prompt_lookup_min .. prompt_lookup_max tokens against the sequence's own past (ngram_propose).  A step then verifies the
    guesses of every live sequence in ONE pass over the weights (td_qwen2_verify_batch_slots) and keeps the sampled tokens up to the first wrong guess
    (td_spec_accept): the tokens are the target model's own draws, a guess only saves passes."""
    method: str = "ngram"
    num_speculative_tokens: int = 3
    prompt_lookup_max: int = 4
    prompt_lookup_min: int = 1

    def validate(self) -> "SpeculativeConfig":
        def bad(field, why):
            raise ValueError(f"SpeculativeConfig.{field}={getattr(self, field)!r}: {why}")

        def integer(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, bool)
        if self.method != "ngram":
            bad("method", 'only "ngram" (prompt lookup) is served: a draft model, EAGLE and Medusa are not built')
        if not (integer(self.num_speculative_tokens) and 1 <= self.num_speculative_tokens <= _hip.MAX_VERIFY_ROWS - 1):
            bad("num_speculative_tokens", f"must be an integer in [1, {_hip.MAX_VERIFY_ROWS - 1}] (a verify step takes {_hip.MAX_VERIFY_ROWS} rows per sequence)")
        if not (integer(self.prompt_lookup_min) and self.prompt_lookup_min >= 1):
            bad("prompt_lookup_min", "must be an integer >= 1")
        if not (integer(self.prompt_lookup_max) and self.prompt_lookup_max >= self.prompt_lookup_min):
            bad("prompt_lookup_max", f"must be an integer >= prompt_lookup_min={self.prompt_lookup_min}")
        return self


def speculative_params_from_vllm_config(vc) -> Optional[SpeculativeConfig]:
    """The SpeculativeConfig a vllm_config asks for with `speculative_config` (None without it).  Any method but "ngram" and any key but
    SPECULATIVE_CONFIG_KEYS is a ValueError naming it: a setting is refused, never ignored."""
    sc = vc.get("speculative_config")
    if sc is None:
        return None
    if not hasattr(sc, "items"):
        raise ValueError(f"vllm_config speculative_config={sc!r}: must be a dict with the keys {SPECULATIVE_CONFIG_KEYS}")
    if sc.get("method", "ngram") != "ngram":
        raise ValueError(f"vllm_config speculative_config method={sc.get('method')!r}: only \"ngram\" is served")
    unknown = sorted(set(sc) - set(SPECULATIVE_CONFIG_KEYS))
    if unknown:
        raise ValueError(f"vllm_config speculative_config sets {unknown}: only {SPECULATIVE_CONFIG_KEYS} are served")
    return SpeculativeConfig(**{k: v for k, v in sc.items() if v is not None}).validate()


def ngram_propose(tokens, n_min: int, n_max: int, k: int) -> np.ndarray:
    """Prompt lookup, the project's statement of the rule (it restates what vLLM's `NgramProposer` computes in `_find_longest_matched_ngram_and_propose_tokens`;
    vLLM itself is not a dependency): take the LONGEST suffix of `tokens`, of length n_max down to n_min, that also occurs earlier in `tokens` (an
    occurrence may overlap the suffix but not be it); of that length use the EARLIEST occurrence; return the up to k tokens that followed it.  Nothing
    matches, or n_min > len(tokens) - 1: an empty array."""
    t = np.asarray(tokens, dtype=np.int64).reshape(-1)
    L = t.size
    if k <= 0:
        return np.empty(0, dtype=np.int32)
    for n in range(min(int(n_max), L - 1), int(n_min) - 1, -1):
        if n < 1:
            break
        suffix = t[L - n:]
        win = np.lib.stride_tricks.sliding_window_view(t[:L - 1], n)      # windows starting at 0 .. L-1-n: every occurrence but the suffix itself
        hit = np.nonzero((win == suffix).all(axis=1))[0]
        if hit.size:
            s0 = int(hit[0]) + n
            return t[s0:s0 + int(k)].astype(np.int32)
    return np.empty(0, dtype=np.int32)


class NgramDraftSource:
    """The draft source of SpeculativeConfig(method="ngram").  A draft source is anything with `propose(token_ids, k) -> ids`: token_ids is a sequence's
    prompt and everything chosen so far (the token about to be fed included), ids up to k guesses for what follows."""

    def __init__(self, config: SpeculativeConfig):
        self.config = config.validate()
        self.k = int(config.num_speculative_tokens)

    def propose(self, token_ids, k):
        return ngram_propose(token_ids, self.config.prompt_lookup_min, self.config.prompt_lookup_max, min(int(k), self.k))


def _draft_source(speculative, what):
    if speculative is None:
        return None
    if isinstance(speculative, SpeculativeConfig):
        return NgramDraftSource(speculative)
    if callable(getattr(speculative, "propose", None)):
        return speculative
    raise ValueError(f"{what}: speculative={speculative!r} must be a SpeculativeConfig or a draft source with propose(token_ids, k)")


def _check_speculative(what, sps, forced):
    """Speculation serves plain sampling only; everything else is refused by name before any GPU work."""
    if forced is not None:
        raise ValueError(f"{what}: speculative= together with forced_output_ids: a teacher-forced continuation has nothing to guess")
    for sp in sps:
        if sp.has_penalty:
            raise ValueError(f"{what}: speculative= together with a penalty (repetition_penalty / presence_penalty / frequency_penalty): the history "
                             "would have to hold the guessed tokens; not built")
        if sp.has_edit:
            raise ValueError(f"{what}: speculative= together with a logit edit (logit_bias / allowed_token_ids / bad_words_token_ids / "
                             "mask_stop_below_min_tokens): not built")
        if sp.logprobs is not None:
            raise ValueError(f"{what}: speculative= together with logprobs={sp.logprobs}: not built")
        if sp.width > 1:
            raise ValueError(f"{what}: speculative= together with n={sp.n}, best_of={sp.best_of}: not built")


Logprob = collections.namedtuple("Logprob", ["logprob", "rank"])      # vLLM's Logprob, without the decoded text


class LogitEditPlan:
    """Which token ids one request bans at which step: vLLM's allowed_token_ids, bad-words and min-tokens rules as set differences, pure Python, no
    device calls (tests/test_logit_edits_cpu.py checks it against a brute-force restatement).

      allowed     allowed_token_ids, or None: everything outside is banned for good (td_logit_edits_allow_only at admission);
      fixed       tokens banned for good: the one-token bad words;
      stops       EOS (unless ignore_eos) and the stop_token_ids, banned while fewer than min_tokens tokens exist (mask_stop_below_min_tokens);
      words       bad words of two or more tokens: the last token is banned at a step iff the request's OUTPUT ends with the word's prefix.
    start() gives the admission-time calls, advance(token) the bans to set and to clear before the next step.  A token is never un-banned while
    another rule still bans it: `fixed` and the complement of `allowed` are never cleared, and the per-step set is kept as one set.  Only a plan with
    `words` needs the sampled token on the host (needs_tokens): every other rule depends on the token COUNT alone, so such requests keep the
    "no host round trip" property of the decode loop."""

    def __init__(self, sp: "SamplingParams", vocab: int, eos_token_id: Optional[int] = None):
        def inside(field, t):
            if int(t) >= vocab:
                raise ValueError(f"SamplingParams.{field}: token id {int(t)} is outside the vocabulary of {vocab} tokens")
            return int(t)
        self.bias = {inside("logit_bias", t): float(v) for t, v in (sp.logit_bias or {}).items()}
        self.allowed = None if sp.allowed_token_ids is None else sorted({inside("allowed_token_ids", t) for t in sp.allowed_token_ids})
        words = [[inside("bad_words_token_ids", t) for t in w] for w in (sp.bad_words_token_ids or [])]
        self.fixed = {w[0] for w in words if len(w) == 1}
        self.words = [w for w in words if len(w) > 1]
        self.min_tokens = int(sp.min_tokens)
        self.stops = set()
        if sp.mask_stop_below_min_tokens and self.min_tokens > 0:
            self.stops = {int(t) for t in (sp.stop_token_ids or []) if 0 <= int(t) < vocab}
            if not sp.ignore_eos and eos_token_id is not None and 0 <= int(eos_token_id) < vocab:
                self.stops.add(int(eos_token_id))
        self.needs_tokens = bool(self.words)
        self.per_step = bool(self.words) or bool(self.stops)
        self._allowed_set = None if self.allowed is None else set(self.allowed)
        self.output: List[int] = []
        self.ngen = 0
        self.current = set()      # what the per-step rules ban now, tokens banned for good left out
        if self.allowed is not None and not (self._allowed_set - self.fixed - self.stops):
            raise ValueError(f"SamplingParams.allowed_token_ids={sp.allowed_token_ids!r}: every allowed token is banned by bad_words_token_ids or the "
                             "min_tokens stop mask, nothing could be sampled")

    def _for_good(self, t):
        return t in self.fixed or (self._allowed_set is not None and t not in self._allowed_set)

    def _wanted(self):
        want = set(self.stops) if self.ngen < self.min_tokens else set()
        for w in self.words:
            k = len(w) - 1
            if k <= len(self.output) and self.output[len(self.output) - k:] == w[:-1]:
                want.add(w[-1])
        return {t for t in want if not self._for_good(t)}

    def start(self):
        """-> (allowed ids or None, ids to ban) for a freshly reset slot, before the first token."""
        self.output, self.ngen = [], 0
        self.current = self._wanted()
        return self.allowed, sorted(self.fixed | self.current)

    def advance(self, token=None):
        """One more token exists (`token`: its id, needed iff needs_tokens) -> (ids to ban, ids to un-ban) before the next step."""
        self.ngen += 1
        if self.needs_tokens:
            self.output.append(int(token))
            del self.output[:-max(len(w) for w in self.words)]      # (only the longest prefix can matter)
        want = self._wanted()
        on, off = sorted(want - self.current), sorted(self.current - want)
        self.current = want
        return on, off


def _sampling_list(sampling, n, what):
    """`sampling` of a generate call -> (one validated SamplingParams per request, rows): rows False = the single-params call whose new fields are
    all at their defaults (td_sample_top_p_bf16, as before); n None: the request count is not known yet (chunks pulled lazily)."""
    if isinstance(sampling, SamplingParams):
        sampling.validate()
        return None, sampling.per_request
    sps = list(sampling)
    if n is not None and len(sps) != n:
        raise ValueError(f"{what}: {len(sps)} SamplingParams for {n} request(s): pass one SamplingParams, or exactly one per request")
    for sp in sps:
        if not isinstance(sp, SamplingParams):
            raise ValueError(f"{what}: sampling must be a SamplingParams or a sequence of them, got {type(sp).__name__}")
        sp.validate()
    return sps, True


def _gather_outputs(seq_res, req_sps):
    """Per-sequence results (k_i = width consecutive entries per request) -> one dict per request.  A request with k = 1 keeps its dict as it is.
    With k > 1 the n returned children -- all of them in child order, or with best_of > n the n highest cumulative logprobs in descending order,
    ties by child index (vLLM V0's rule) -- become "outputs": dicts with "index", "token_ids", "hidden_states", "cumulative_logprob" when the
    children were scored or logprobs were asked, and "logprobs" only when asked; the generate()-style keys describe output 0 and
    "prompt_hidden_states" is the one shared prefill's."""
    out, s0 = [], 0
    for sp in req_sps:
        k = sp.width
        kids, s0 = seq_res[s0:s0 + k], s0 + k
        if k == 1:
            out.append(kids[0])
            continue
        order = sorted(range(k), key=lambda j: (-kids[j]["cumulative_logprob"], j))[:sp.n] if k > sp.n else list(range(k))
        outs = []
        for idx, j in enumerate(order):
            o = {"index": idx, "token_ids": kids[j]["token_ids"], "hidden_states": kids[j]["hidden_states"]}
            if "cumulative_logprob" in kids[j]:
                o["cumulative_logprob"] = kids[j]["cumulative_logprob"]
            if sp.logprobs is not None:
                o["logprobs"] = kids[j]["logprobs"]
            outs.append(o)
        r = {"prompt_hidden_states": kids[0]["prompt_hidden_states"]}
        r.update({key: v for key, v in outs[0].items() if key != "index"})
        r["outputs"] = outs
        out.append(r)
    return out


class _RowSampling:
    """The per-request sampler path of one generate call (td_sample_rows_bf16): a device table of TdSampleRow structs in live-row order, rewritten only
    when the live set changes, and the offsets uploaded per step.  A request with its own seed draws from (seed, its generated-token count, 0), so
    its tokens do not depend on which rows share the step; the others draw from (the call's key, the step, live row) as the single-params path does.
    History (the engine's td_sampler, created on first use) is kept only for requests with a penalty; every other row names slot -1.
    Logit edits (the engine's td_logit_edits, created on first use, one slot per cache slot): a request with an edit (SamplingParams.has_edit) has
    its slot reset and filled at admission from its LogitEditPlan, names that slot in the per-row edit-slot table, and has the plan's per-step ban
    changes applied after every token (advance).  A step none of whose live rows has an edit calls sample_rows exactly as before.  Only a request
    with a bad word of two or more tokens needs its sampled token on the host every step; everything else depends on token counts alone."""

    def __init__(self, engine, key, eos_token_id=None):
        self.engine, self.key, self.eos = engine, int(key), eos_token_id
        self.table, self.seeded, self.state = None, [], None
        self.plans, self.edit_slots, self.live_plans = {}, None, []

    def admit(self, slot, sp, prompt_ids):
        if sp.has_penalty:
            self.engine._sampler_state().reset_slot(int(slot), [int(t) for t in prompt_ids])
        self.plans.pop(int(slot), None)
        if sp.has_edit:
            plan = LogitEditPlan(sp, self.engine.config.vocab_size, self.eos)      # (raises ValueError for an id outside the vocabulary, before any device call)
            ed = self.engine._logit_edits()
            ed.reset_slot(int(slot))      # a reused slot starts clean
            allowed, ban = plan.start()
            if allowed is not None:
                ed.allow_only(int(slot), allowed)
            if ban:
                ed.ban(int(slot), ban, True)
            if plan.bias:
                ed.set_bias(int(slot), plan.bias)
            self.plans[int(slot)] = plan

    def set_live(self, rows):
        """rows: (SamplingParams, cache slot) per live row."""
        recs, self.seeded, any_hist = [], [], False
        es = [int(slot) if int(slot) in self.plans and sp.has_edit else -1 for sp, slot in rows]
        self.live_plans = [(i, s, self.plans[s]) for i, s in enumerate(es) if s >= 0 and self.plans[s].per_step]
        self.edit_slots = torch.tensor(es, dtype=torch.int32).to(self.engine.device) if any(s >= 0 for s in es) else None
        for r, (sp, slot) in enumerate(rows):
            hist = sp.has_penalty
            any_hist |= hist
            self.seeded.append(sp.seed is not None)
            recs.append(dict(temperature=sp.temperature, top_p=sp.top_p, min_p=sp.min_p, repetition_penalty=sp.repetition_penalty,
                             presence_penalty=sp.presence_penalty, frequency_penalty=sp.frequency_penalty, top_k=sp.top_k,
                             slot=int(slot) if hist else -1, stream=0 if sp.seed is not None else r,
                             seed=sp.seed if sp.seed is not None else self.key))
        self.table = _hip.pack_sample_rows(recs).to(self.engine.device)
        self.state = self.engine._sampler_state().handle if any_hist else None

    def sample(self, logits, step, ngen):
        """logits [n, vocab] of the live rows; step: the call's decode step; ngen[i]: tokens live row i has generated."""
        offs = torch.tensor([int(ngen[i]) if s else int(step) for i, s in enumerate(self.seeded)], dtype=torch.int64).to(self.engine.device)
        if self.edit_slots is None:
            return _OPS.sample_rows(logits, self.table, offs, self.state, self.state is not None)
        return _OPS.sample_rows_edit(logits, self.table, offs, self.state, self.state is not None, self.engine._logit_edits().handle, self.edit_slots)

    def advance(self, toks):
        """After a step: toks[i] is live row i's new token (a device tensor, a list or an array; read on the host only for the rows whose plan has a
        bad word of several tokens).  Applies each plan's ban changes to its edit slot before the next step's launch."""
        if not self.live_plans:
            return
        ed = self.engine._logit_edits()
        for i, slot, plan in self.live_plans:
            on, off = plan.advance(int(toks[i]) if plan.needs_tokens else None)
            if off:
                ed.ban(slot, off, False)
            if on:
                ed.ban(slot, on, True)


class _LogprobLog:
    """The logprobs of one generate call (td_logprobs_rows_bf16 on the RAW logits of every step, one launch per step for the rows that asked): the
    results stay on the device and are read once at the end.  add(): logits [n, vocab], the n chosen (sampled or forced) tokens as a device int32
    tensor, and the request each row belongs to; finish(): res[i]["logprobs"] = per generated token a dict token_id -> Logprob(logprob, rank) holding
    the chosen token and the top `logprobs` ones (ranks 1, 2, .. in the kernel's order), res[i]["cumulative_logprob"] = the sum over the chosen
    tokens -- for the requests that asked, nobody else's dict changes."""

    def __init__(self, engine, want):
        """want: SamplingParams.logprobs per request (None: not asked), a list, or one int for every request."""
        self.engine = engine
        self.want = (lambda i, v=int(want): v) if isinstance(want, numbers.Integral) else (lambda i, w=list(want): w[i])
        self.cap = int(want) if isinstance(want, numbers.Integral) else max([0] + [int(v) for v in want if v is not None])
        self.steps = []

    @staticmethod
    def wanted(sps):
        return any(sp.logprobs is not None for sp in sps)

    def add(self, logits, tok_dev, owners):
        n_top = [-1 if self.want(int(o)) is None else int(self.want(int(o))) for o in owners]
        if max(n_top) < 0:
            return
        x = logits if logits.dim() == 2 else logits[None]
        out = _OPS.logprobs_rows(x, tok_dev.to(torch.int32), torch.tensor(n_top, dtype=torch.int32).to(self.engine.device), self.cap)
        self.steps.append(([int(o) for o in owners], tok_dev, n_top, out))

    def finish(self, res):
        for i, r in enumerate(res):
            if self.want(i) is not None:
                r["logprobs"], r["cumulative_logprob"] = [], 0.0
        if not self.steps:
            return
        toks = torch.cat([s[1].to(torch.int32).reshape(-1) for s in self.steps]).cpu().tolist()
        lp, rank, tid, tlp = (torch.cat([s[3][j] for s in self.steps]).cpu().tolist() for j in range(4))
        r0 = 0
        for owners, _, n_top, _ in self.steps:
            for i, (o, n) in enumerate(zip(owners, n_top)):
                if n >= 0:
                    k = r0 + i
                    d = {int(tid[k][j]): Logprob(float(tlp[k][j]), j + 1) for j in range(n)}
                    d[int(toks[k])] = Logprob(float(lp[k]), int(rank[k]))
                    res[o]["logprobs"].append(d)
                    res[o]["cumulative_logprob"] += float(lp[k])
            r0 += len(owners)


class _TokenSource:
    """Where the tokens of one generate call's steps come from, for all three entries: the teacher-forced ids, the per-request sampler (_RowSampling,
    admitted per slot, its table rewritten lazily after the live set changed) or the one plain launch (td_sample_top_p_bf16) under the call's ONE
    sampler key, and the logprobs of what was chosen (_LogprobLog).  sp_of(s): the SamplingParams of sequence s; forced[s]: its forced ids (None: the
    call samples); want: SamplingParams.logprobs per sequence, one int for every sequence, or None when nobody asked."""

    def __init__(self, engine, sampling, by_rows, sp_of, eos_token_id, generator, forced, want, draft=None):
        self.engine, self.sampling, self.sp_of, self.forced = engine, sampling, sp_of, forced
        self.draft = draft      # speculative decoding: the draft source (None: every step is one token per sequence, exactly as before)
        self.spec_table = None
        if draft is not None:
            engine._spec_stats = dict(steps=0, drafted=0, accepted=0, emitted=0)
        self.key = None if forced is not None else engine._draw_sampler_key(generator)
        self.rows = _RowSampling(engine, self.key, eos_token_id) if by_rows and forced is None else None      # (forced decoding does not sample and keeps no history)
        self.lplog = _LogprobLog(engine, want) if want is not None else None      # (forced tokens are scored too)
        self.live_changed = True

    def admit(self, slot, sp, prompt_ids):
        """A sequence starts in cache slot `slot`: that slot's history and logit edits start over."""
        if self.rows is not None:
            self.rows.admit(slot, sp, prompt_ids)
        self.live_changed = True

    def next(self, logits, step, ngen, owners, slots):
        """logits [n, vocab] of the live rows; step: the call's decode step; ngen[i], owners[i], slots[i]: tokens generated so far, sequence and cache
        slot of live row i.  -> (device int32 [n] tokens, the same ids as a host array where the host already holds them -- forced ids, or a bad
        word of several tokens had them read -- else None: a caller that needs them downloads them itself)."""
        host = None
        if self.forced is not None:
            host = np.array([self.forced[o][g] for o, g in zip(owners, ngen)], dtype=np.int32)
            tok = torch.from_numpy(host).to(self.engine.device)
        elif self.rows is not None:
            if self.live_changed:
                self.rows.set_live([(self.sp_of(int(o)), int(s)) for o, s in zip(owners, slots)])
            tok = self.rows.sample(logits, step, ngen)
            if any(plan.needs_tokens for _, _, plan in self.rows.live_plans):
                host = tok.cpu().numpy()
            self.rows.advance(tok if host is None else host)
        else:
            tok = _OPS.sample_top_p(logits, float(self.sampling.temperature), float(self.sampling.top_p), int(self.key), int(step))
        self.live_changed = False
        if self.lplog is not None:
            self.lplog.add(logits, tok, owners)
        return tok, host

    def spec_sample(self, logits, owners, live_of_row, offsets):
        """Speculative decoding: one sampler launch (td_sample_rows_bf16) over rows that belong to live sequences live_of_row[r] (several rows per
        sequence in a verify step).  A seeded sequence draws token number g at (seed, g, 0), as on the plain path; the others at (the call's key, g,
        sequence index) -- NOT the plain path's (key, step, live row): a step no longer emits one token per sequence, so the step does not name a
        token.  offsets[r]: the number g of the token row r's logits choose."""
        if self.live_changed or self.spec_table is None:
            recs = []
            for o in owners:
                sp = self.sp_of(int(o))
                recs.append(dict(temperature=sp.temperature, top_p=sp.top_p, min_p=sp.min_p, top_k=sp.top_k, slot=-1,
                                 stream=0 if sp.seed is not None else int(o), seed=sp.seed if sp.seed is not None else self.key))
            self.spec_table = _hip.pack_sample_rows(recs)
            self.live_changed = False
        table = self.spec_table if len(live_of_row) == len(owners) else self.spec_table.index_select(0, torch.from_numpy(np.asarray(live_of_row, dtype=np.int64)))
        return _OPS.sample_rows(logits, table.to(self.engine.device), torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(self.engine.device), None, False)

    def finish(self, res):
        """res[s]["logprobs"] and ["cumulative_logprob"] of the sequences that asked: present only then."""
        if self.lplog is not None:
            self.lplog.finish(res)


class _LiveRows:
    """The live sequences of generate_batch and generate_continuous and their one decode step.  Per live row (numpy, rows [0, n)): sequence, cache
    slot, cached tokens, next position id, tokens generated, token budget, min_tokens and stop ids; logits[i] = the next-token logits of live row i.
    The per-step bookkeeping is vectorised and the arrays are handed to the C ABI as they are: at 256 sequences the Python-list form cost ~2 ms of
    host time per step, about as much as the step takes on the GPU, which idles while the host prepares the next launch.  The hidden rows of a step
    stay ONE device tensor and are handed to their sequences by a single gather after the loop (results).

    What the two entries do differently is all in what they pass to admit() and when they call it:
      budget           generate_batch: min(max_tokens, len(forced ids)), and a sequence with budget 0 is prefilled but never live; generate_continuous:
                       len(forced ids) alone under forced ids, and a request with budget 0 is never admitted (a prompt-only forward);
      sampler offsets  the step counts every decode step of the call and seeded rows draw at their own token count: generate_batch admits once, so
                       both are its loop index; generate_continuous admits between steps, so they differ;
      slot capacity    both retire a sequence silently when its slot is full (generate, the single-sequence entry, lets the native check raise);
      prompts          a prompt that fits no prefill pass is served by generate_batch (one forward) and refused by generate_continuous."""

    def __init__(self, engine, capacity, source, eos_token_id):
        self.engine, self.src, self.eos = engine, source, eos_token_id
        self.own, self.slt, self.clen, self.npos, self.ngen, self.lim, self.mint = (np.zeros(capacity, dtype=np.int32) for _ in range(7))
        self.stops = np.empty(capacity, dtype=object)
        # speculative decoding (source.draft): per live row the token chosen but not yet fed (-1: none, its next-token logits are in self.logits) and
        # the prompt + every token chosen so far, which the draft source reads
        self.pend = np.full(capacity, -1, dtype=np.int32)
        self.hist = np.empty(capacity, dtype=object)
        self.n, self.step_no, self.any_stop = 0, 0, False
        self.logits = torch.empty(capacity, engine.config.vocab_size, dtype=torch.bfloat16, device=engine.device)
        self.step_hid, self.step_owner, self.step_toks = [], [], []

    def admit(self, seq0, widths, slots, lens, npos, budgets, prompts, free_slots):
        """k requests were just prefilled: request j into cache slot slots[j], lens[j] prompt tokens, generation continuing at position npos[j], its
        prefill logits in self.logits[n + j].  It runs as the sequences seq0[j] .. seq0[j] + widths[j] - 1 with budgets[j] tokens each: the first
        on its slot, the children (n / best_of) on the next slots popped from free_slots -- after all k parents took theirs -- which start from a copy
        of the prompt's cache rows (one launch per request, td_qwen2_fork_slot) and of its row of logits."""
        n, k, used = self.n, len(slots), sum(widths)
        rep = [j for j in range(k) for _ in range(widths[j])]
        seqs = [s for j in range(k) for s in range(seq0[j], seq0[j] + widths[j])]
        if used > k:
            seq_slots = []
            for j in range(k):
                kids = [free_slots.pop() for _ in range(widths[j] - 1)]
                if kids:
                    self.engine._fork_slots(slots[j], kids, lens[j])
                    self.engine._lora_inherit(slots[j], kids)
                seq_slots += [slots[j]] + kids
            self.logits[n:n + used] = self.logits[n:n + k].index_select(0, torch.tensor(rep, dtype=torch.int64).to(self.logits.device))
            slots = seq_slots
        sps = [self.src.sp_of(s) for s in seqs]
        for sp, sl, j in zip(sps, slots, rep):
            self.src.admit(sl, sp, prompts[j])
        live = [r for r, j in enumerate(rep) if budgets[j] > 0]
        if len(live) < used:
            self.logits[n:n + len(live)] = self.logits[n:n + used].index_select(0, torch.tensor(live, dtype=torch.int64).to(self.logits.device))
        m = n + len(live)
        self.own[n:m] = [seqs[r] for r in live]
        self.slt[n:m] = [slots[r] for r in live]
        self.clen[n:m] = [lens[rep[r]] for r in live]
        self.npos[n:m] = [npos[rep[r]] for r in live]
        self.ngen[n:m] = 0
        self.lim[n:m] = [budgets[rep[r]] for r in live]
        self.mint[n:m] = [sps[r].min_tokens for r in live]
        self.pend[n:m] = -1
        for i, r in zip(range(n, m), live):      # (forced ids run to their end: no stop rule)
            sp = sps[r]
            if self.src.draft is not None:
                self.hist[i] = [int(t) for t in prompts[rep[r]]]
            self.stops[i] = set() if self.src.forced is not None else \
                set(sp.stop_token_ids or []) | ({self.eos} if not sp.ignore_eos and self.eos is not None else set())
            self.any_stop |= bool(self.stops[i])
        self.n = m

    def step(self):
        """One token for every live sequence: choose it, decode it (one pass over the weights, td_qwen2_decode_batch_slots), apply the stop rule
        and close the gaps of the finished rows (the order of the others is kept: no cache rows move).  -> the freed cache slots, highest first."""
        if self.src.draft is not None:
            return self._spec_step()
        n, dev = self.n, self.engine.device
        tok_dev, toks = self.src.next(self.logits[:n], self.step_no, self.ngen[:n], self.own[:n], self.slt[:n])
        if toks is None:
            toks = tok_dev.cpu().numpy()      # (the host sees the ids once per step, for the stop rule and the results)
        return self._feed_one(tok_dev, toks)

    def _feed_one(self, tok_dev, toks):
        """The plain step behind the choice of its tokens: decode one token per live sequence, stop rule, retire."""
        n, dev = self.n, self.engine.device
        pos_dev = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(self.npos[:n], (3, n)))).to(dev)
        hid = torch.empty(n, self.engine.config.hidden_size, dtype=torch.bfloat16, device=dev)
        self.engine._decode_slots(n, self.slt, tok_dev, pos_dev, self.clen, hid, self.logits)      # logits of row i -> logits[i]
        self.step_hid.append(hid)
        self.step_owner.append(self.own[:n].copy())
        self.step_toks.append(toks)
        self.clen[:n] += 1
        self.npos[:n] += 1
        self.ngen[:n] += 1
        self.step_no += 1
        done = (self.ngen[:n] >= self.lim[:n]) | (self.clen[:n] >= self.engine.slot_len)
        if self.any_stop:
            hit = np.fromiter((int(t) in s for t, s in zip(toks, self.stops[:n])), dtype=bool, count=n)
            done |= hit & (self.ngen[:n] >= self.mint[:n])
        return self._retire(done)

    def _retire(self, done):
        """Close the gaps of the finished rows.  -> the freed cache slots, highest first."""
        n, dev = self.n, self.engine.device
        if not done.any():
            return []
        keep = np.nonzero(~done)[0]
        freed = sorted((int(x) for x in self.slt[:n][done]), reverse=True)
        self.engine._lora_release(freed)
        k = keep.size
        for arr in (self.own, self.slt, self.clen, self.npos, self.ngen, self.lim, self.mint, self.stops, self.pend, self.hist):
            arr[:k] = arr[:n][keep]
        if k:
            self.logits[:k] = self.logits[:n].index_select(0, torch.from_numpy(keep).to(dev))
        self.src.live_changed = True
        self.n = k
        return freed

    def _spec_step(self):
        """The step under speculative decoding.  Every live sequence holds one chosen-but-unfed token (drawn here from its next-token logits where it
        has none), the draft source guesses what follows, and ONE pass over the weights feeds [that token | guesses] of every sequence
        (td_qwen2_verify_batch_slots).  All rows are sampled in one launch, td_spec_accept keeps the samples up to the first wrong guess, the host reads
        (n_emit, emit) once.  Row 0 and the rows of the accepted guesses were computed on a true prefix: their hidden states and tokens are the
        sequence's, token by token under the stop rule; the last emitted sample is the next step's unfed token.  Rejected rows stay in the cache and
        are overwritten by the next step.  A step in which nobody has a guess is the plain step."""
        n, dev, eng, src = self.n, self.engine.device, self.engine, self.src
        stats = eng._spec_stats
        need = self.pend[:n] < 0
        if need.any():
            t0 = src.spec_sample(self.logits[:n], self.own[:n], np.arange(n), self.ngen[:n]).cpu().numpy()
            self.pend[:n] = np.where(need, t0, self.pend[:n])
        # guesses: at most the token budget less the unfed token, the slot's free rows less one, 7, and what keeps the step inside 256 rows
        row_cap = eng.MAX_BATCH // n - 1
        drafts = []
        for i in range(n):
            room = min(int(self.lim[i] - self.ngen[i]) - 1, eng.slot_len - int(self.clen[i]) - 1, _hip.MAX_VERIFY_ROWS - 1, row_cap)
            d = []
            if room > 0:
                self.hist[i].append(int(self.pend[i]))
                d = [int(t) for t in np.asarray(src.draft.propose(self.hist[i], room)).reshape(-1)[:room]]
                self.hist[i].pop()
            drafts.append(d)
        stats["steps"] += 1
        if not any(drafts):
            toks = self.pend[:n].copy()
            self.pend[:n] = -1
            for i in range(n):
                self.hist[i].append(int(toks[i]))
            stats["emitted"] += n
            return self._feed_one(torch.from_numpy(toks).to(dev), toks)
        n_new = np.array([1 + len(d) for d in drafts], dtype=np.int32)
        row0 = np.concatenate([[0], np.cumsum(n_new)[:-1]]).astype(np.int32)
        R = int(n_new.sum())
        fed = np.concatenate([[self.pend[i]] + drafts[i] for i in range(n)]).astype(np.int32)
        live_of_row = np.repeat(np.arange(n), n_new)
        within = np.arange(R) - row0[live_of_row]
        pos = (self.npos[:n][live_of_row] + within).astype(np.int32)
        fed_dev = torch.from_numpy(fed).to(dev)
        pos_dev = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(pos, (3, R)))).to(dev)
        hid = torch.empty(R, eng.config.hidden_size, dtype=torch.bfloat16, device=dev)
        lg = torch.empty(R, eng.config.vocab_size, dtype=torch.bfloat16, device=dev)
        eng._verify_slots(n, self.slt, n_new, fed_dev, pos_dev, self.clen, hid, lg)
        sampled = src.spec_sample(lg, self.own[:n], live_of_row, self.ngen[:n][live_of_row] + 1 + within)
        n_emit, emit = _OPS.spec_accept(sampled, fed_dev, torch.from_numpy(row0).to(dev), torch.from_numpy(n_new).to(dev))
        got = torch.cat([n_emit.reshape(n, 1), emit.reshape(n, -1)], dim=1).cpu().numpy()      # (the step's one download)
        done = np.zeros(n, dtype=bool)
        rows_kept, owners_kept, toks_kept = [], [], []
        for i in range(n):
            a = int(got[i, 0]) - 1
            stats["drafted"] += len(drafts[i])
            stats["accepted"] += a
            keep = 0
            for j in range(a + 1):      # the fed tokens on a true prefix, one at a time as the plain loop would have met them
                tok = int(fed[row0[i] + j])
                keep += 1
                g = int(self.ngen[i]) + keep
                if g >= self.lim[i] or int(self.clen[i]) + keep >= eng.slot_len or (tok in self.stops[i] and g >= self.mint[i]):
                    done[i] = True
                    break
            rows_kept.extend(range(int(row0[i]), int(row0[i]) + keep))
            owners_kept.extend([int(self.own[i])] * keep)
            toks_kept.extend(fed[row0[i]:row0[i] + keep].tolist())
            self.hist[i].extend(fed[row0[i]:row0[i] + keep].tolist())
            self.clen[i] += keep
            self.npos[i] += keep
            self.ngen[i] += keep
            self.pend[i] = int(got[i, 1 + a])
            stats["emitted"] += keep
        self.step_hid.append(hid if len(rows_kept) == R else hid.index_select(0, torch.tensor(rows_kept, dtype=torch.int64).to(dev)))
        self.step_owner.append(np.array(owners_kept, dtype=np.int32))
        self.step_toks.append(np.array(toks_kept, dtype=np.int32))
        self.step_no += 1
        return self._retire(done)

    def results(self, res):
        """res[s]["hidden_states"] and ["token_ids"] of every sequence s (one gather: rows grouped by sequence, in step order inside a sequence),
        then the logprobs of those that asked."""
        D, dev = self.engine.config.hidden_size, self.engine.device
        if self.step_owner:
            owners_all = np.concatenate(self.step_owner)
            order = np.argsort(owners_all, kind="stable")
            counts = np.bincount(owners_all, minlength=len(res)).tolist()
            parts = torch.split(torch.cat(self.step_hid).index_select(0, torch.from_numpy(order).to(dev)), counts)
            toks_sorted = np.concatenate(self.step_toks)[order].tolist()
            r0 = 0
            for r, part, c in zip(res, parts, counts):
                r["hidden_states"], r["token_ids"] = part, toks_sorted[r0:r0 + c]
                r0 += c
        else:
            for r in res:
                r["hidden_states"] = torch.empty(0, D, dtype=torch.bfloat16, device=dev)
        self.src.finish(res)


class Qwen2VLTextEngine:
    dtype = torch.bfloat16

    # vLLM's `kv_cache_dtype` values the engine serves: "auto" (the model dtype, bf16) and the two spellings of OCP e4m3
    KV_CACHE_DTYPES = {"auto": _hip.QWEN2_KV_BF16, "fp8": _hip.QWEN2_KV_E4M3, "fp8_e4m3": _hip.QWEN2_KV_E4M3}

    @classmethod
    def check_kv_cache_dtype(cls, value):
        """vllm_config["kv_cache_dtype"] as the models take it: "auto" / None (bf16), "fp8" or "fp8_e4m3" (the e4m3 cache); anything else -- "fp8_e5m2"
        included -- is an error naming the value, never ignored.  Returns "auto" or "fp8"."""
        if value is None:
            return "auto"
        if not isinstance(value, str) or value not in cls.KV_CACHE_DTYPES:
            raise ValueError(f"vllm_config kv_cache_dtype={value!r} is not served by the HIP engine: only 'fp8' / 'fp8_e4m3' (e4m3 bytes with a power-of-two "
                             "scale per token and kv head), or 'auto' / None for bf16")
        return "auto" if cls.KV_CACHE_DTYPES[value] == _hip.QWEN2_KV_BF16 else "fp8"

    def __init__(self, config: Optional[Qwen2VLTextConfig] = None, max_model_len: int = 8192, device="cuda", n_slots: int = 1,
                 prefill_rows: Optional[int] = None, kv_cache_dtype: Optional[str] = "auto", enable_prefix_caching: bool = False,
                 enable_lora: bool = False, max_loras: int = 1, max_lora_rank: int = 16, **kw):
        self.kv_cache_dtype = self.check_kv_cache_dtype(kv_cache_dtype)      # (before anything is allocated)
        self.check_prefix_caching(enable_prefix_caching)
        if not isinstance(enable_lora, bool):
            raise ValueError(f"enable_lora={enable_lora!r} must be True or False")
        if enable_lora:
            _lora.check_pool_size(max_loras, max_lora_rank)
        self.config = config or Qwen2VLTextConfig(**kw)
        c = self.config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _hip.ThinkDiffHipError("Qwen2VLTextEngine runs on the MI355X HIP engine only (device='cuda')")
        self._L = _hip.lib()
        cc = _hip.TdQwen2Config(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, 128,
                                c.intermediate_size, c.vocab_size, int(c.tie_word_embeddings),
                                (ctypes.c_int * 3)(*c.mrope_section), c.rms_norm_eps, c.rope_theta)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            # n_slots sequences of max_model_len tokens each (batched decode); n_slots = 1 is the single-request engine
            # prefill_rows: activation-workspace rows = the capacity (sum of padded prompt lengths) of one batched prefill
            self.prefill_rows = max(int(prefill_rows or 0), max_model_len)
            _hip.check(self._L.td_qwen2_create_kv(ctypes.byref(cc), max_model_len, int(n_slots), self.prefill_rows,
                                                  self.KV_CACHE_DTYPES[self.kv_cache_dtype], ctypes.byref(h)))
        self._h = h
        # set by the models from vllm_config["quantization"]: every load below then ends with quantize_weights (None: the bf16 engine, untouched)
        self.weight_quantization: Optional[str] = None
        self.int4_config: Optional[dict] = None      # an AWQ / GPTQ checkpoint's own `quantization_config` (load_pretrained reads it from config.json)
        self._defer_quantize = False
        self.n_slots, self.slot_len = int(n_slots), max_model_len
        self.max_model_len = max_model_len
        self.set_prefix_caching(enable_prefix_caching)
        self._lora = None
        if enable_lora:      # vLLM's enable_lora: the adapter pool and the low-rank kernels' workspace (td_qwen2_lora_enable), once, here
            with torch.cuda.device(self.device):
                _hip.check(self._L.td_qwen2_lora_enable(self._h, int(max_loras), int(max_lora_rank)))
            self._lora = _lora.LoraPool(int(max_loras), int(max_lora_rank), self._lora_dev_load, self._lora_dev_remove, self._lora_dev_set_slot)

    # ---- per-request LoRA (vLLM's enable_lora / LoRARequest; thinkdiff/models/qwen2_lora.py) ------------------------------------------------------
    def _lora_dev_load(self, place: int, adapter):
        for (layer, module), (A, B) in adapter.pairs.items():
            a, b = A.to(self.device), B.to(self.device)
            _hip.check(self._L.td_qwen2_lora_load(self._h, int(place), f"model.layers.{layer}.{module}".encode(), _hip.ptr(a), _hip.ptr(b), int(adapter.rank),
                                                  float(adapter.scale), _hip.stream_ptr()))

    def _lora_dev_remove(self, place: int):
        _hip.check(self._L.td_qwen2_lora_remove(self._h, int(place)))

    def _lora_dev_set_slot(self, slot: int, place: int):
        _hip.check(self._L.td_qwen2_lora_set_slot(self._h, int(slot), int(place)))

    def _lora_pool(self, what):
        pool = getattr(self, "_lora", None)
        if pool is None:
            raise ValueError(f"{what}: LoRA was requested on an engine created without enable_lora=True")
        return pool

    def add_lora(self, request_or_name, state_dict=None, config=None) -> bool:
        """vLLM's `LLM.add_lora`: register an adapter.  request_or_name: a LoRARequest (or a dict of its fields), or a name -- the adapter then gets the next
        free lora_int_id.  state_dict + config: the adapter in peft's published layout and its adapter_config.json as a dict; without them the adapter is read
        from the request's lora_path (a peft directory).  Tensors of another float dtype are rounded to bf16 once, here.  It reaches the device at its first
        use (or now, while the pool has a free place).  Returns True; see thinkdiff/models/qwen2_lora.py for what is refused."""
        pool = self._lora_pool("add_lora")
        if isinstance(request_or_name, str):
            req = LoRARequest(request_or_name, max(list(pool.known) + [0]) + 1)
        else:
            req = LoRARequest.of(request_or_name)
        if req is None:
            raise ValueError("add_lora: a LoRARequest or a name is required")
        if state_dict is None:
            if req.lora_path is None:
                raise ValueError(f"add_lora: adapter {req.lora_int_id} ('{req.lora_name}') comes with neither a state_dict nor a lora_path")
            state_dict, config = _lora.load_adapter_dir(req.lora_path)
        elif config is None:
            raise ValueError("add_lora: a state_dict needs its config dict (peft's adapter_config.json: r, lora_alpha, ...)")
        adapter = _lora.parse_adapter(state_dict, config, _lora.module_shapes(self.config), self.config.num_hidden_layers, pool.max_lora_rank)
        pool.register(req, adapter)
        if len(pool.resident) < pool.max_loras:
            pool.place([req.lora_int_id])
        return True

    def remove_lora(self, lora_int_id: int) -> bool:
        """vLLM's `LLM.remove_lora`: forget the adapter (device and host).  A later request naming it must bring a lora_path.  -> whether it was known."""
        return self._lora_pool("remove_lora").forget(int(lora_int_id))

    def list_loras(self) -> List[int]:
        """vLLM's `LLM.list_loras`: the ids of the registered adapters."""
        pool = getattr(self, "_lora", None)
        return [] if pool is None else sorted(pool.known)

    def lora_info(self) -> dict:
        """max_loras (0: not enabled), resident adapters, bytes the pool and the kernels' workspace hold, low-rank launches enqueued or captured so far
        (td_qwen2_lora_info), and the pool's loads / evictions."""
        m, r, b, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        _hip.check(self._L.td_qwen2_lora_info(self._h, ctypes.byref(m), ctypes.byref(r), ctypes.byref(b), ctypes.byref(n)))
        pool = getattr(self, "_lora", None)
        return {"max_loras": m.value, "resident": r.value, "bytes": b.value, "launches": n.value, **({} if pool is None else pool.stats)}

    def _lora_req_of(self, request) -> Optional[LoRARequest]:
        """The adapter a request dict names (key "lora_request": a LoRARequest or a dict of its fields), known to the pool: one that was never added is read
        from its lora_path now."""
        req = LoRARequest.of(request.get("lora_request"))
        if req is None:
            return None
        pool = self._lora_pool("lora_request")
        if req.lora_int_id not in pool.known:
            if req.lora_path is None:
                raise ValueError(f"lora_request: adapter {req.lora_int_id} ('{req.lora_name}') is not loaded (add_lora) and names no lora_path")
            self.add_lora(req)
        return req

    def _lora_check_call(self, requests):
        """A call whose requests name more distinct adapters than max_loras is refused before anything runs."""
        reqs = [self._lora_req_of(r) for r in requests]
        if any(r is not None for r in reqs):
            self._lora_pool("lora_request").check_call(reqs)

    def _lora_bind(self, requests, slots):
        """In front of a prefill: cache slot slots[j] runs under request j's adapter (none: under none), the adapter resident."""
        reqs = [self._lora_req_of(r) for r in requests]
        pool = getattr(self, "_lora", None)
        if pool is not None:
            pool.bind([int(x) for x in slots], reqs)

    def _lora_inherit(self, src, dst_slots):
        pool = getattr(self, "_lora", None)
        if pool is not None:
            pool.inherit(src, dst_slots)

    def _lora_release(self, slots):
        pool = getattr(self, "_lora", None)
        if pool is not None:
            pool.release(slots)

    # ---- automatic prefix caching (vLLM's enable_prefix_caching; thinkdiff/models/prefix_cache.py) ----------------------------------------------
    @staticmethod
    def check_prefix_caching(value) -> bool:
        """vllm_config["enable_prefix_caching"] as the models take it: a bool; anything else is an error naming the value."""
        if not isinstance(value, bool):
            raise ValueError(f"vllm_config enable_prefix_caching={value!r} must be True or False")
        return value

    def set_prefix_caching(self, on: bool):
        """Turn automatic prefix caching on or off (off by default; turning it off forgets everything).  On: generate_batch, generate_continuous, beam_search
        and the n / best_of parents serve the longest cached run of whole 16-token blocks of a prompt from a donor cache slot and prefill the rest."""
        on = self.check_prefix_caching(on)
        if on and getattr(self, "_prefix_cache", None) is None:
            self._prefix_cache = _pfx.PrefixCache(self.n_slots)
        elif not on:
            self._prefix_cache = None
        return self

    def reset_prefix_cache(self):
        """vLLM's LLM.reset_prefix_cache: every slot forgets its prompt (the statistics keep counting)."""
        pc = getattr(self, "_prefix_cache", None)
        if pc is not None:
            pc.resize(self.n_slots)
        return self

    def prefix_cache_stats(self) -> dict:
        """queries / hits in tokens (vLLM's metrics), passes, copies (launches) and copied_rows, in_place take-overs, deferred requests, evictions, and
        hidden_bytes: the prompts' hidden rows the entries hold on the device.  All zero while the feature is off."""
        pc = getattr(self, "_prefix_cache", None)
        return _pfx.zero_stats() if pc is None else pc.get_stats()

    def _pc_wrote(self, slots):
        """A low-level writer called from outside the generate entries wrote these slots: their cached prompts are gone."""
        pc = getattr(self, "_prefix_cache", None)
        if pc is not None and not getattr(self, "_pc_depth", 0):
            for s in slots:
                pc.drop(int(s))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.td_qwen2_destroy(h)
        st, self._sampler = getattr(self, "_sampler", None), None
        if st is not None:
            st.close()
        ed, self._edits = getattr(self, "_edits", None), None
        if ed is not None:
            ed.close()

    def _logit_edits(self):
        """The edit slots behind logit_bias, allowed_token_ids, bad words and the min_tokens stop mask (td_logit_edits, one slot per cache slot),
        created the first time a request with an edit arrives: n_slots x (2 x vocab / 8 + 8196) bytes of device memory (11.8 MB at 256 x 152 064)."""
        ed = getattr(self, "_edits", None)
        if ed is None or ed.n_slots != max(1, self.n_slots):
            if ed is not None:
                ed.close()
            ed = self._edits = _hip.LogitEdits(max(1, self.n_slots), self.config.vocab_size, self.device)
        return ed

    def _sampler_state(self):
        """The token history behind the penalties (td_sampler, one slot per cache slot), created the first time a request with a penalty arrives:
        n_slots x vocab x 2.25 bytes of device memory (87.6 MB at 256 x 152 064)."""
        st = getattr(self, "_sampler", None)
        if st is None or st.n_slots != max(1, self.n_slots):
            if st is not None:
                st.close()
            st = self._sampler = _hip.Sampler(max(1, self.n_slots), self.config.vocab_size, self.device)
        return st

    # ---- parameters (Hugging Face names) -----------------------------------------------------------------
    def param_table(self) -> Dict[str, int]:
        buf, cnt, out = ctypes.create_string_buffer(256), ctypes.c_int64(), {}
        for i in range(self._L.td_qwen2_num_params(self._h)):
            _hip.check(self._L.td_qwen2_param_info(self._h, i, buf, 256, ctypes.byref(cnt)))
            out[buf.value.decode()] = cnt.value
        return out

    def _dequantize_packed(self, sd: Dict[str, torch.Tensor], table: Dict[str, int]) -> Dict[str, torch.Tensor]:
        """A pre-quantised MXFP4 checkpoint (Quark / torchao layout): a decoder Linear or lm_head given as `<name>.weight` uint8 [N, K / 2] plus
        `<name>.weight_scale` uint8 [N, K / 32] is dequantised EXACTLY to bf16 here and loaded like any weight; the quantisation that closes the load
        rebuilds the engine's copy from those values, which it reproduces bit for bit whatever scale rule wrote the checkpoint (every e2m1 value times
        2, 4 or 8 is on the grid again).  Anything malformed is a ValueError naming the key."""
        packed = [k for k, t in sd.items() if k in table and k.endswith(".weight") and t.dtype == torch.uint8]
        for k in sd:
            if k.endswith(".weight_scale") and k[:-len("_scale")] not in packed:
                raise ValueError(f"Qwen2VLTextEngine.load_state_dict: {k!r} has no packed uint8 tensor {k[:-len('_scale')]!r} beside it")
        if not packed:
            return sd
        out = {k: t for k, t in sd.items() if not k.endswith(".weight_scale")}
        for k in packed:
            if self.weight_quantization != "mxfp4":
                raise ValueError(f"Qwen2VLTextEngine.load_state_dict: {k!r} is a packed MXFP4 tensor but the engine's quantization is "
                                 f"{self.weight_quantization!r}: packed weights load only with quantization='mxfp4'")
            if k + "_scale" not in sd:
                raise ValueError(f"Qwen2VLTextEngine.load_state_dict: packed MXFP4 tensor {k!r} lacks its scales {k + '_scale'!r}")
            q, sc = sd[k], sd[k + "_scale"]
            K = 2 * q.shape[-1] if q.dim() == 2 else 0
            if q.dim() != 2 or K % 32 != 0 or q.numel() * 2 != table[k] or k.split(".")[-2] not in self.PACKED_LINEARS:
                raise ValueError(f"Qwen2VLTextEngine.load_state_dict: packed MXFP4 tensor {k!r} has shape {tuple(q.shape)}: expected uint8 [N, K / 2] "
                                 f"with N K = {table[k]} and K a multiple of 32, on a decoder Linear or lm_head")
            if sc.dtype != torch.uint8 or tuple(sc.shape) != (q.shape[0], K // 32):
                raise ValueError(f"Qwen2VLTextEngine.load_state_dict: {k + '_scale'!r} is {sc.dtype} {tuple(sc.shape)}: expected uint8 "
                                 f"{(q.shape[0], K // 32)} (one e8m0 byte per 32 weights of a row)")
            out[k] = _hip.dequant_rows_mxfp4(q.to(self.device).contiguous(), sc.to(self.device).contiguous())
        return out

    # the Linears a packed checkpoint may carry: the ones quantize_weights("mxfp4") quantises
    PACKED_LINEARS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj", "lm_head")

    # the Linears an AWQ / GPTQ checkpoint quantises (lm_head and the embedding table stay bf16 there), and the tensors such a Linear comes as
    INT4_LINEARS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
    INT4_TENSORS = ("qweight", "qzeros", "scales", "g_idx")

    @staticmethod
    def check_int4_config(cfg) -> dict:
        """An AWQ / GPTQ checkpoint's `quantization_config` as the engine serves it -> {"layout": td_repack_int4's, "group_size": G}; anything else is a
        ValueError naming the field.  Served: 4 bits, group_size 32 / 64 / 128; AWQ version "gemm" with zero points; GPTQ without act-order
        (checkpoint_format "gptq" or "gptq_v2")."""
        def bad(field, why):
            return ValueError(f"Qwen2VLTextEngine: int4_config[{field!r}]={cfg.get(field)!r} is not served by the HIP engine: {why}")
        if not isinstance(cfg, dict):
            raise ValueError(f"Qwen2VLTextEngine: int4_config must be the checkpoint's quantization_config dict, got {type(cfg).__name__}")
        method = cfg.get("quant_method")
        if method not in ("awq", "gptq"):
            raise bad("quant_method", "'awq' and 'gptq' are the int4 checkpoint formats it loads")
        if cfg.get("bits") != 4:
            raise bad("bits", "only 4-bit checkpoints (3- and 8-bit GPTQ are not built)")
        G = cfg.get("group_size")
        if G not in _hip.INT4_GROUP_SIZES:
            raise bad("group_size", f"the group sizes served are {_hip.INT4_GROUP_SIZES} (no per-channel -1)")
        if method == "awq":
            if str(cfg.get("version", "gemm")).lower() != "gemm":
                raise bad("version", "only AutoAWQ's 'gemm' layout (no 'gemv' / Marlin)")
            if cfg.get("zero_point", True) is not True:
                raise bad("zero_point", "the AWQ layout it reads carries zero points")
            return {"layout": _hip.INT4_AWQ, "group_size": G}
        if cfg.get("desc_act", False):
            raise bad("desc_act", "act-order (a g_idx other than k // group_size) is not built")
        fmt = cfg.get("checkpoint_format", "gptq")
        if fmt not in ("gptq", "gptq_v2"):
            raise bad("checkpoint_format", "'gptq' and 'gptq_v2' are the ones read (no Marlin)")
        return {"layout": _hip.INT4_GPTQ | (_hip.INT4_GPTQ_V2 if fmt == "gptq_v2" else 0), "group_size": G}

    def _split_int4(self, sd: Dict[str, torch.Tensor], table: Dict[str, int]):
        """An AWQ / GPTQ state dict: a decoder Linear given as `<linear>.qweight` + `.qzeros` + `.scales` (+ `.g_idx`) instead of `.weight`.
        -> (the dict without those tensors, [(weight name, layout, G, qweight, qzeros, scales)]).  Everything is checked here, on the host, before any
        device work; anything malformed or unserved is a ValueError naming the key or the config field."""
        me = "Qwen2VLTextEngine.load_state_dict"
        bases = []
        for k in sd:
            base, _, suffix = k.rpartition(".")
            if suffix in self.INT4_TENSORS and (base + ".weight" in table or base == "lm_head") and base not in bases:
                bases.append(base)
        if not bases:
            return sd, []
        if "lm_head" in bases:
            key = next(k for k in sd if k.startswith("lm_head.") and k.rpartition(".")[2] in self.INT4_TENSORS)
            raise ValueError(f"{me}: {key!r}: a quantised lm_head is not served (AWQ / GPTQ Qwen2-VL checkpoints keep lm_head and the embeddings in bf16)")
        if self.int4_config is None:
            raise ValueError(f"{me}: {bases[0] + '.qweight'!r} is an AWQ / GPTQ int4 tensor, but the engine has no int4_config (the checkpoint's "
                             "quantization_config; load_pretrained reads it from config.json)")
        if self.weight_quantization is not None:
            raise ValueError(f"{me}: int4 tensors ({bases[0] + '.qweight'!r}) cannot be combined with weight_quantization={self.weight_quantization!r}: "
                             "the checkpoint is quantised already, and one engine holds one weight format")
        spec = self.check_int4_config(self.int4_config)
        layout, G = spec["layout"], spec["group_size"]
        awq = layout == _hip.INT4_AWQ
        jobs = []
        for base in bases:
            name = base + ".weight"
            if base.split(".")[-1] not in self.INT4_LINEARS:
                raise ValueError(f"{me}: {base + '.qweight'!r}: only the decoder Linears {self.INT4_LINEARS} load as int4")
            if name in sd:
                raise ValueError(f"{me}: {name!r} is given both as bf16 and as int4 tensors")
            for suffix in ("qweight", "qzeros", "scales"):
                if base + "." + suffix not in sd:
                    raise ValueError(f"{me}: int4 Linear {base!r} lacks {base + '.' + suffix!r}")
            qw, qz, sc = sd[base + ".qweight"], sd[base + ".qzeros"], sd[base + ".scales"]
            if qw.dtype != torch.int32 or qw.dim() != 2:
                raise ValueError(f"{me}: {base + '.qweight'!r} is {qw.dtype} {tuple(qw.shape)}: expected a 2-D int32 tensor")
            K, N = (qw.shape[0], qw.shape[1] * 8) if awq else (qw.shape[0] * 8, qw.shape[1])
            if N * K != table[name] or K % G != 0 or K % 32 != 0 or N % 8 != 0:
                raise ValueError(f"{me}: {base + '.qweight'!r} has shape {tuple(qw.shape)}: expected int32 "
                                 f"{'[K, N / 8]' if awq else '[K / 8, N]'} with N K = {table[name]}, K a multiple of group_size {G} and of 32, N of 8")
            if qz.dtype != torch.int32 or tuple(qz.shape) != (K // G, N // 8):
                raise ValueError(f"{me}: {base + '.qzeros'!r} is {qz.dtype} {tuple(qz.shape)}: expected int32 {(K // G, N // 8)}")
            if sc.dtype != torch.float16:
                raise ValueError(f"{me}: {base + '.scales'!r} is {sc.dtype}: the scales must be float16 (bf16 scales are not served)")
            if tuple(sc.shape) != (K // G, N):
                raise ValueError(f"{me}: {base + '.scales'!r} has shape {tuple(sc.shape)}: expected float16 {(K // G, N)}")
            if not bool(torch.isfinite(sc).all()):
                raise ValueError(f"{me}: {base + '.scales'!r} holds a non-finite scale")
            if base + ".g_idx" in sd:
                gi = sd[base + ".g_idx"]
                if awq or tuple(gi.shape) != (K,) or not torch.equal(gi.to("cpu", torch.int64), torch.arange(K) // G):
                    raise ValueError(f"{me}: {base + '.g_idx'!r} is not the map k // group_size of a GPTQ checkpoint without act-order (desc_act is not built)")
            jobs.append((name, layout, G, qw, qz, sc))
        drop = {b + "." + t for b in bases for t in self.INT4_TENSORS}
        return {k: t for k, t in sd.items() if k not in drop}, jobs

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        self.reset_prefix_cache()      # (the cached keys and hidden rows belong to the old weights)
        table = self.param_table()
        sd, int4_jobs = self._split_int4(sd, table)
        sd = self._dequantize_packed(sd, table)
        as_int4 = {job[0] for job in int4_jobs}
        missing = [k for k in table if k not in sd and k not in as_int4]
        if strict and missing:
            raise KeyError(f"Qwen2VLTextEngine.load_state_dict: missing {missing[:4]}..")
        for name, layout, G, qw, qz, sc in int4_jobs:      # repacked into the device layout, then into the arena (as W^) and the handle's int4 copy
            dev = [t.to(self.device).contiguous() for t in (qw, qz, sc)]
            packed, scales, zeros = _hip.repack_int4(layout, dev[0], dev[1], dev[2], G)
            _hip.check(self._L.td_qwen2_load_param_int4(self._h, name.encode(), _hip.ptr(packed), _hip.ptr(scales), _hip.ptr(zeros), G, _hip.stream_ptr()))
            torch.cuda.current_stream().synchronize()
        for name, t in sd.items():
            if name in table:
                d = t.to(device=self.device, dtype=torch.bfloat16).contiguous()
                _hip.check(self._L.td_qwen2_load_param(self._h, name.encode(), _hip.ptr(d), d.numel(), _hip.stream_ptr()))
                torch.cuda.current_stream().synchronize()
        self._requantize()
        return missing

    def _requantize(self):
        # a quantised engine whose parameters changed refuses to run until it is quantised again: do it here rather than leave the handle stale
        if self.weight_quantization and not self._defer_quantize:
            self.quantize_weights(self.weight_quantization)

    def load_pretrained(self, path: str):
        """Text-decoder tensors of a LOCAL Hugging Face Qwen2-VL checkpoint directory (*.safetensors; `visual.*` skipped).  A config.json beside the
        shards whose `quantization_config` says quant_method "awq" or "gptq" (the published Qwen2-VL-*-Instruct-AWQ / -GPTQ-Int4) becomes `int4_config`
        and the decoder Linears load as int4 -- what vLLM does with `quantization` left unset."""
        import glob
        import json
        import os
        from safetensors import safe_open
        files = sorted(glob.glob(os.path.join(path, "*.safetensors")))
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {path}")
        cfg_path = os.path.join(path, "config.json")
        if os.path.exists(cfg_path):
            with open(cfg_path) as fh:
                qc = json.load(fh).get("quantization_config")
            if isinstance(qc, dict) and qc.get("quant_method") in ("awq", "gptq"):
                self.check_int4_config(qc)
                self.int4_config = qc
        if self.int4_config is not None:      # one dict for all shards: the three tensors of a Linear need not share a shard
            sd = {}
            for fn in files:
                with safe_open(fn, framework="pt") as fh:
                    for k in fh.keys():
                        if "visual." not in k:
                            sd[k.replace("model.language_model.", "model.")] = fh.get_tensor(k)
            missing = [k for k in self.load_state_dict(sd, strict=False) if not (k == "lm_head.weight" and self.config.tie_word_embeddings)]
            if missing:
                raise KeyError(f"checkpoint at {path} lacks {len(missing)} decoder tensors, e.g. {missing[:3]}")
            return self
        seen = set()
        self._defer_quantize = True      # (one quantisation behind the last shard, not one per shard)
        try:
            for fn in files:
                with safe_open(fn, framework="pt") as fh:
                    sd = {}
                    for k in fh.keys():
                        if "visual." in k:
                            continue
                        name = k.replace("model.language_model.", "model.")     # newer exports nest the decoder
                        sd[name] = fh.get_tensor(k)
                    seen.update(sd)
                    self.load_state_dict(sd, strict=False)
        finally:
            self._defer_quantize = False
        missing = [k for k in self.param_table() if k not in seen and not (k == "lm_head.weight" and self.config.tie_word_embeddings)]
        if missing:
            raise KeyError(f"checkpoint at {path} lacks {len(missing)} decoder tensors, e.g. {missing[:3]}")
        self._requantize()
        return self

    def init_random(self, seed: int = 0, std: float = 0.02):
        self.reset_prefix_cache()
        _hip.check(self._L.td_qwen2_init_random(self._h, seed, std, _hip.stream_ptr()))
        self._requantize()
        return self

    # ---- 8-bit weight stream --------------------------------------------------------------------------------
    WEIGHT_QUANTIZATIONS = {"fp8": _hip.QWEN2_WEIGHTS_E4M3, "mxfp4": _hip.QWEN2_WEIGHTS_MXFP4}

    @classmethod
    def check_quantization(cls, value):
        """vllm_config["quantization"] as the models take it: None (bf16), "fp8" or "mxfp4"; anything else is an error, never ignored."""
        if value is not None and value not in cls.WEIGHT_QUANTIZATIONS:
            raise ValueError(f"vllm_config quantization={value!r} is not served by the HIP engine: only 'fp8' (weight-only e4m3) and 'mxfp4' "
                             "(weight-only OCP MXFP4), or None for bf16.  AWQ / GPTQ int4 checkpoints are recognised from their own quantization_config "
                             "(config.json beside the shards) with quantization left unset")
        return value

    def quantize_weights(self, quantization: str = "fp8"):
        """Weight-only fp8 of every decoder Linear and lm_head (vLLM's `quantization="fp8"`): e4m3 bytes with one power-of-two scale per output row
        beside the bf16 weights, which are OVERWRITTEN with the dequantised values (exactly representable; with tied embeddings the embedding table too).
        Decode steps of up to 64 sequences then stream the bytes; prefill and wider steps run the same model in bf16.  Call after the weights
        are loaded, and again after any later load_state_dict / init_random (runs are refused until then).
        "mxfp4" (vLLM's `quantization="mxfp4"`) is the same scheme in OCP MXFP4: e2m1 nibbles under one e8m0 scale per 32 weights of a row, 0.27x the
        bf16 bytes, its dequantised values exact in bf16 too.  An engine quantised in one format refuses the other until its weights are loaded again."""
        if quantization not in Qwen2VLTextEngine.WEIGHT_QUANTIZATIONS:
            raise ValueError(f"Qwen2VLTextEngine.quantize_weights: quantization={quantization!r} is not served (only 'fp8' and 'mxfp4')")
        self.reset_prefix_cache()
        _hip.check(self._L.td_qwen2_quantize_weights(self._h, Qwen2VLTextEngine.WEIGHT_QUANTIZATIONS[quantization], _hip.stream_ptr()))
        return self

    def set_weight_stream(self, on: bool) -> bool:
        """A/B switch of a quantised engine: launches of up to 64 rows read the 8-bit copy (default) or the dequantised bf16 weights -- the same
        model either way.  Returns the previous setting."""
        self.reset_prefix_cache()
        rc = self._L.td_qwen2_set_weight_stream(self._h, 1 if on else 0)
        if rc not in (0, 1):
            _hip.check(rc)
        return bool(rc)

    def set_int4_routing(self, all_rows: bool) -> bool:
        """Measurement and test switch of an int4 engine: with the stream on, every launch of up to 64 rows reads the int4 copy (True) or only the row
        counts at which the int4 forms measured faster than the bf16 kernels (False, the default) -- the same model either way.  Returns the previous
        setting."""
        rc = self._L.td_qwen2_set_int4_routing(self._h, 1 if all_rows else 0)
        if rc not in (0, 1):
            _hip.check(rc)
        return bool(rc)

    def weight_stream_launches(self) -> int:
        """Linear launches enqueued so far that read the 8-bit copy (a captured decode step counts when captured, not per replay)."""
        return int(self._L.td_qwen2_weight_stream_launches(self._h))

    def weight_info(self) -> dict:
        mode, on, nbytes, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int()
        _hip.check(self._L.td_qwen2_weight_info(self._h, ctypes.byref(mode), ctypes.byref(on), ctypes.byref(nbytes), ctypes.byref(n)))
        names = {**{v: k for k, v in self.WEIGHT_QUANTIZATIONS.items()}, _hip.QWEN2_WEIGHTS_INT4: "int4"}      # (int4: loaded, never quantised here)
        return {"mode": names.get(mode.value, "bf16"), "stream_on": bool(on.value),
                "bytes_8bit": int(nbytes.value), "n_linears": int(n.value)}

    # ---- e4m3 KV cache ----------------------------------------------------------------------------------------
    def kv_cache_info(self) -> dict:
        """{"dtype": "auto" | "fp8", "bytes_per_row": bytes of one cache row of one layer, "cache_bytes": bytes of the whole handle's cache}."""
        mode, row, total = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        _hip.check(self._L.td_qwen2_kv_info(self._h, ctypes.byref(mode), ctypes.byref(row), ctypes.byref(total)))
        return {"dtype": "fp8" if mode.value == _hip.QWEN2_KV_E4M3 else "auto", "bytes_per_row": int(row.value), "cache_bytes": int(total.value)}

    def read_kv(self, layer: int, slot: int, row0: int, n: int) -> torch.Tensor:
        """Cache rows [row0, row0 + n) of sequence `slot` in layer `layer` as bf16 [n, 2 Hkv 128] (rotated k heads | v heads): the values every
        consumer sees -- on an e4m3 cache the dequantised bytes, which is exact."""
        out = torch.empty(int(n), 2 * self.config.num_key_value_heads * 128, dtype=torch.bfloat16, device=self.device)
        _hip.check(self._L.td_qwen2_read_kv(self._h, int(layer), int(slot), int(row0), int(n), _hip.ptr(out), _hip.stream_ptr()))
        return out

    # ---- one decoder pass over n new tokens ---------------------------------------------------------------
    def set_slots(self, n_slots: int):
        """Split the KV cache into `n_slots` sequences (each max_model_len // n_slots tokens) for batched decode."""
        _hip.check(self._L.td_qwen2_set_slots(self._h, int(n_slots)))
        self.n_slots, self.slot_len = int(n_slots), int(self._L.td_qwen2_slot_capacity(self._h))
        self.reset_prefix_cache()      # (the slots' rows moved)
        if getattr(self, "_lora", None) is not None:
            self._lora.clear_slots()
        return self

    def set_fused_rope(self, on: bool) -> bool:
        """Decode step: rotary embedding + cache write inside the attention launch (default) or as a launch of their own.  Returns the
        previous setting."""
        return bool(self._L.td_qwen2_set_fused_rope(self._h, 1 if on else 0))

    def forward(self, position_ids, token_ids=None, inputs_embeds=None, pos0: int = 0, want_hidden=True, want_logits=False, slot: int = 0, lora_request=_KEEP):
        """position_ids int32 [3,n]; token_ids int32 [n] or inputs_embeds bf16 [n,hidden].  Returns
        (hidden [n,hidden] | None, logits_last [vocab] | None).  lora_request: a LoRARequest -- the slot runs under that adapter from here on (this call,
        decode_batch and verify_batch rows naming the slot) -- or None: under none; not given: as the slot stands."""
        if lora_request is not _KEEP:
            self._lora_bind([{"lora_request": lora_request}], [slot])
        pos = position_ids.to(self.device, torch.int32).contiguous()
        n = pos.shape[1]
        tok = None if token_ids is None else token_ids.to(self.device, torch.int32).contiguous()
        emb = None if inputs_embeds is None else inputs_embeds.to(self.device, torch.bfloat16).contiguous()
        hid = torch.empty(n, self.config.hidden_size, dtype=torch.bfloat16, device=self.device) if want_hidden else None
        lg = torch.empty(self.config.vocab_size, dtype=torch.bfloat16, device=self.device) if want_logits else None
        self._pc_wrote([slot])
        _hip.check(self._L.td_qwen2_forward_slot(self._h, slot, _hip.ptr(tok), _hip.ptr(emb), _hip.ptr(pos), n, pos0,
                                                 _hip.ptr(hid), _hip.ptr(lg), _hip.stream_ptr()))
        return hid, lg

    def decode_batch(self, token_ids, position_ids, cache_pos: Sequence[int], want_logits=True, slots: Optional[Sequence[int]] = None):
        """One token for each of the sequences in cache slots `slots` (default 0..B-1) in a single pass over the weights.
        token_ids [B], position_ids [3,B], cache_pos[b] = tokens already cached.  -> (hidden [B,hidden], logits [B,vocab] | None)."""
        B = len(cache_pos)
        tok = torch.as_tensor(token_ids, dtype=torch.int32).to(self.device).contiguous()
        pos = torch.as_tensor(position_ids, dtype=torch.int32).to(self.device).contiguous()
        assert tok.shape == (B,) and pos.shape == (3, B)
        hid = torch.empty(B, self.config.hidden_size, dtype=torch.bfloat16, device=self.device)
        lg = torch.empty(B, self.config.vocab_size, dtype=torch.bfloat16, device=self.device) if want_logits else None
        cp = (ctypes.c_int * B)(*[int(c) for c in cache_pos])
        sl = ctypes.cast((ctypes.c_int * B)(*[int(c) for c in slots]), ctypes.c_void_p) if slots is not None else None
        self._pc_wrote(slots if slots is not None else range(B))
        _hip.check(self._L.td_qwen2_decode_batch_slots(self._h, B, sl, _hip.ptr(tok), _hip.ptr(pos), ctypes.cast(cp, ctypes.c_void_p),
                                                       _hip.ptr(hid), _hip.ptr(lg), _hip.stream_ptr()))
        return hid, lg

    def verify_batch(self, token_ids, position_ids, cache_pos: Sequence[int], n_new: Sequence[int], slots: Optional[Sequence[int]] = None, want_logits=True):
        """The verify step of speculative decoding (td_qwen2_verify_batch_slots): sequence b feeds n_new[b] tokens (1..8) at cache rows cache_pos[b] ..,
        R = sum(n_new) rows, sequence after sequence.  token_ids [R], position_ids [3, R].  -> (hidden [R, hidden], logits [R, vocab] | None): row
        (b, j) is what decode_batch returns for that token after the j tokens before it.  All R cache rows are written; the caller advances by what it
        keeps."""
        B, R = len(cache_pos), int(sum(int(v) for v in n_new))
        tok = torch.as_tensor(token_ids, dtype=torch.int32).to(self.device).contiguous()
        pos = torch.as_tensor(position_ids, dtype=torch.int32).to(self.device).contiguous()
        if len(n_new) != B or tok.shape != (R,) or pos.shape != (3, R):
            raise _hip.ThinkDiffHipError(f"verify_batch: {len(n_new)} n_new for {B} sequences, token_ids {tuple(tok.shape)} and position_ids {tuple(pos.shape)} for R={R} rows")
        hid = torch.empty(R, self.config.hidden_size, dtype=torch.bfloat16, device=self.device)
        lg = torch.empty(R, self.config.vocab_size, dtype=torch.bfloat16, device=self.device) if want_logits else None
        cp = (ctypes.c_int * B)(*[int(c) for c in cache_pos])
        nn = (ctypes.c_int * B)(*[int(c) for c in n_new])
        sl = ctypes.cast((ctypes.c_int * B)(*[int(c) for c in slots]), ctypes.c_void_p) if slots is not None else None
        self._pc_wrote(slots if slots is not None else range(B))
        _hip.check(self._L.td_qwen2_verify_batch_slots(self._h, B, sl, ctypes.cast(nn, ctypes.c_void_p), _hip.ptr(tok), _hip.ptr(pos),
                                                       ctypes.cast(cp, ctypes.c_void_p), _hip.ptr(hid), _hip.ptr(lg), _hip.stream_ptr()))
        return hid, lg

    # ---- multimodal prompt assembly ([ext] vLLM Qwen2-VL input processor + transformers Qwen2VLModel.get_rope_index) ----
    def embed_tokens(self, token_ids) -> torch.Tensor:
        """[n] ids -> bf16 [n, hidden] rows of model.embed_tokens."""
        tok = torch.as_tensor(token_ids, dtype=torch.int32).to(self.device).contiguous()
        out = torch.empty(tok.numel(), self.config.hidden_size, dtype=torch.bfloat16, device=self.device)
        _hip.check(self._L.td_qwen2_embed_tokens(self._h, _hip.ptr(tok), _hip.ptr(out), tok.numel(), _hip.stream_ptr()))
        return out

    @staticmethod
    def expand_image_placeholders(token_ids: Sequence[int], grid_thw, merge: int = 2, image_token_id: int = 151655) -> List[int]:
        """Each `<|image_pad|>` in the templated prompt stands for one image: repeat it t*h*w/merge^2 times (one per
        merged vision token).  Prompts whose placeholders are already expanded pass through unchanged."""
        counts = [int(t) * int(h) * int(w) // (merge * merge) for t, h, w in grid_thw]
        ids = list(token_ids)
        if sum(1 for v in ids if v == image_token_id) == sum(counts):
            return ids
        if sum(1 for v in ids if v == image_token_id) != len(counts):
            raise ValueError(f"prompt holds {sum(1 for v in ids if v == image_token_id)} image placeholders for {len(counts)} images")
        out, k = [], 0
        for v in ids:
            if v == image_token_id:
                out.extend([v] * counts[k])
                k += 1
            else:
                out.append(v)
        return out

    @staticmethod
    def mrope_position_ids(token_ids: Sequence[int], grid_thw, merge: int = 2, image_token_id: int = 151655) -> torch.Tensor:
        """int32 [3, n] (t, h, w) streams: text runs count up on all three; an image block keeps t fixed and walks
        its merged (h/merge, w/merge) grid; the text after it resumes at max + 1."""
        ids = list(token_ids)
        pos = torch.zeros(3, len(ids), dtype=torch.int32)
        i, nxt, img = 0, 0, 0
        while i < len(ids):
            if ids[i] == image_token_id:
                t, h, w = (int(v) for v in grid_thw[img])
                gh, gw = h // merge, w // merge
                n = t * gh * gw
                pos[0, i:i + n] = nxt + torch.arange(t, dtype=torch.int32).repeat_interleave(gh * gw)
                pos[1, i:i + n] = nxt + torch.arange(gh, dtype=torch.int32).repeat_interleave(gw).repeat(t)
                pos[2, i:i + n] = nxt + torch.arange(gw, dtype=torch.int32).repeat(t * gh)
                nxt += max(t, gh, gw)
                i += n
                img += 1
            else:
                pos[:, i] = nxt
                nxt += 1
                i += 1
        return pos

    @staticmethod
    def text_position_ids(n: int, start: int = 0) -> torch.Tensor:
        return (torch.arange(n, dtype=torch.int32) + start)[None, :].expand(3, n).contiguous()

    # ---- the part of LLM.generate(return_hidden_states=True) the reference consumes ------------------------
    @torch.no_grad()
    def generate(self, prompt_token_ids: Sequence[int], sampling: SamplingParams, position_ids=None, inputs_embeds=None,
                 eos_token_id: Optional[int] = None, generator: Optional[torch.Generator] = None,
                 forced_output_ids: Optional[Sequence[int]] = None, speculative=None, lora_request=None):
        """Returns dict(prompt_hidden_states [n_prompt,D], hidden_states [n_gen,D], token_ids [n_gen]).
        speculative: a SpeculativeConfig or a draft source -- the batch path then runs the one sequence (generate_batch).
        lora_request: the LoRARequest the sequence runs under (vLLM's `generate(..., lora_request=)`).

        Sampling is temperature / top-p on the device.  `forced_output_ids` teacher-forces the continuation
        (the reference samples at T=0.6, so parity of the hidden states is checked on forced ids)."""
        sps, by_rows = _sampling_list(sampling, 1, "generate")
        if sps is not None:
            sampling = sps[0]
        if speculative is not None:
            _draft_source(speculative, "generate")
            _check_speculative("generate", [sampling], forced_output_ids)
            return self.generate_batch([{"prompt_token_ids": prompt_token_ids, "position_ids": position_ids, "inputs_embeds": inputs_embeds,
                                         "lora_request": lora_request}], sampling, eos_token_id=eos_token_id, generator=generator, speculative=speculative)[0]
        if sampling.width > 1:      # n / best_of: one prefill, k sequences on forked slots -- the batch path runs them
            if forced_output_ids is not None:
                raise ValueError(f"generate: forced_output_ids with SamplingParams n={sampling.n}, best_of={sampling.best_of}: a teacher-forced "
                                 "continuation is one sequence")
            if self.n_slots < sampling.width:
                raise _hip.ThinkDiffHipError(f"generate: SamplingParams n={sampling.n}, best_of={sampling.best_of} needs {sampling.width} cache slots, "
                                             f"n_slots={self.n_slots}; call set_slots first")
            return self.generate_batch([{"prompt_token_ids": prompt_token_ids, "position_ids": position_ids, "inputs_embeds": inputs_embeds,
                                         "lora_request": lora_request}], sampling, eos_token_id=eos_token_id, generator=generator)[0]
        n_p = len(prompt_token_ids)
        pos = self.text_position_ids(n_p) if position_ids is None else position_ids
        next_pos = int(pos.max()) + 1      # M-RoPE: generation continues one past the largest prompt position
        tok = torch.tensor(list(prompt_token_ids), dtype=torch.int32)
        if lora_request is not None or getattr(self, "_lora", None) is not None:
            self._lora_bind([{"lora_request": lora_request}], [0])
        prompt_hidden, lg = self.forward(pos, tok if inputs_embeds is None else None, inputs_embeds, 0, True, True)
        logits = lg[None]
        out_tok, out_hidden = [], []
        forced = forced_output_ids
        stops = set(sampling.stop_token_ids or []) | ({eos_token_id} if not sampling.ignore_eos and eos_token_id is not None else set())
        src = _TokenSource(self, sampling, by_rows, lambda s: sampling, eos_token_id, generator, None if forced is None else [forced],
                           None if sampling.logprobs is None else [sampling.logprobs])
        src.admit(0, sampling, prompt_token_ids)
        for step in range(sampling.max_tokens if forced is None else min(sampling.max_tokens, len(forced))):
            nxt, host = src.next(logits, step, [step], [0], [0])      # device int32 [1], no host round trip
            out_tok.append(nxt)
            # one token against the cache: the decode step (fused rope + cache write, decode attention, gated-MLP weight stream).  Unlike the batched
            # entries nothing here looks at the slot's capacity: a sequence that outgrows its slot raises from the native check
            h1, logits = self.decode_batch(nxt, [[next_pos + step]] * 3, [n_p + step])
            out_hidden.append(h1)
            if forced is None and stops and step + 1 >= sampling.min_tokens:      # only now does the host need to see the token
                if int(nxt if host is None else host[0]) in stops:
                    break
        hs = torch.cat(out_hidden) if out_hidden else torch.empty(0, self.config.hidden_size, dtype=torch.bfloat16, device=self.device)
        out_ids = torch.cat(out_tok).tolist() if out_tok else []
        res = {"prompt_hidden_states": prompt_hidden, "hidden_states": hs, "token_ids": out_ids}
        src.finish([res])
        if not getattr(self, "_lora_depth", 0):
            self._lora_release([0])
        return res

    @staticmethod
    def _draw_sampler_key(generator: Optional[torch.Generator] = None) -> int:
        """64-bit key of one generate() call's sampling stream, drawn from `generator` (default: torch's global CPU generator),
        so `torch.manual_seed` / a seeded generator reproduce the sampled tokens and successive calls differ.  The HIP sampler
        derives row r's draw for generated token t from (key, t, r) (td_sample_top_p_bf16)."""
        dev = generator.device if generator is not None else "cpu"
        return int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=dev))

    packed_prefill = True   # _prefill_prompts: prompts back to back (td_qwen2_prefill_packed_slots); False = right-padded (generate_batch) or one forward per prompt
    MAX_BATCH = 256     # td_qwen2_decode_batch: sequences sharing one decode step (vLLM's max_num_seqs of the precompute job)
    n_slots = 1         # (until __init__ / set_slots say otherwise)

    @property
    def max_seqs(self) -> int:
        """Sequences one call can keep live: one cache slot each, and one decode step takes at most MAX_BATCH."""
        return min(self.MAX_BATCH, self.n_slots)

    @_prefix_entry
    @torch.no_grad()
    def generate_batch(self, requests: Sequence[dict], sampling: SamplingParams, eos_token_id: Optional[int] = None,
                       generator: Optional[torch.Generator] = None, forced_output_ids: Optional[Sequence[Sequence[int]]] = None, speculative=None):
        """`generate` for up to min(256, n_slots) requests together: each prompt is prefilled into its own cache slot, then
        every decode step advances all unfinished sequences in one pass over the weights (what vLLM's batching gives the
        reference's precompute job).  requests: dicts with "prompt_token_ids" and optional "position_ids" / "inputs_embeds".
        A request's "lora_request" (a LoRARequest) names the adapter its sequences run under.  Returns one generate()-style dict per request, in order."""
        B, forced = len(requests), forced_output_ids
        self._lora_check_call(requests)
        sps, by_rows = _sampling_list(sampling, B, "generate_batch")
        if sps is None:
            sps = [sampling] * B
        draft = _draft_source(speculative, "generate_batch")
        if draft is not None:
            _check_speculative("generate_batch", sps, forced)
        if B > self.max_seqs:
            raise _hip.ThinkDiffHipError(f"generate_batch: {B} requests exceed min({self.MAX_BATCH}, n_slots={self.n_slots}); call set_slots first")
        widths = [sp.width for sp in sps]      # n / best_of: request b runs as widths[b] sequences, each on a cache slot of its own
        N, fan = sum(widths), max(widths, default=1) > 1
        if fan and forced is not None:
            raise ValueError("generate_batch: forced_output_ids with SamplingParams n / best_of > 1: a teacher-forced continuation is one sequence")
        if N > self.max_seqs:
            raise _hip.ThinkDiffHipError(f"generate_batch: the requests' n / best_of add up to {N} sequences, which exceed "
                                         f"min({self.MAX_BATCH}, n_slots={self.n_slots}); call set_slots first")
        # sequences are numbered in request order; `res`, the live rows and the logprob log are per sequence, _gather_outputs hands them back
        seq_sps = [c for sp in sps for c in sp.children()]
        seq0 = np.concatenate([[0], np.cumsum(widths)]).tolist()
        res = [{"prompt_hidden_states": None, "hidden_states": None, "token_ids": []} for _ in range(N)]
        poss = [self._positions(r) for r in requests]
        src = _TokenSource(self, sampling, by_rows, seq_sps.__getitem__, eos_token_id, generator, forced,
                           [sp.logprobs for sp in seq_sps] if _LogprobLog.wanted(seq_sps) else None, draft)
        live = _LiveRows(self, N, src, eos_token_id)
        pc = getattr(self, "_prefix_cache", None)
        if pc is None:
            # request b is prefilled once, into slot b; the children take the slots from B up
            parents, free_slots = list(range(B)), list(range(N - 1, B - 1, -1))
            hidden = self._prefill_prompts(requests, parents, poss, live.logits[:B], padded_ok=True)
        else:      # prefix caching: the cache places the prompts and hands out the children's slots; a finished sequence's slot is retained
            free_slots = _CacheSlots(pc)
            hidden, parents = self._prefill_prompts_cached(pc, requests, poss, live.logits[:B])
        for b, h in enumerate(hidden):
            res[seq0[b]]["prompt_hidden_states"] = h
        live.admit(seq0, widths, parents, [len(r["prompt_token_ids"]) for r in requests], [int(p.max()) + 1 for p in poss],
                   [sp.max_tokens if forced is None else min(sp.max_tokens, len(forced[b])) for b, sp in enumerate(sps)],
                   [r["prompt_token_ids"] for r in requests], free_slots)
        while live.n:
            freed = live.step()
            if pc is not None:
                free_slots.extend(freed)
        live.results(res)
        return _gather_outputs(res, sps) if fan else res

    @_prefix_entry
    @torch.no_grad()
    def generate_continuous(self, request_chunks, sampling: SamplingParams, eos_token_id: Optional[int] = None,
                            generator: Optional[torch.Generator] = None, forced_output_ids: Optional[Sequence[Sequence[int]]] = None,
                            max_live: Optional[int] = None, admit_min: Optional[int] = None, speculative=None):
        """Continuous batching ([ext] vLLM's scheduler behind the reference's `LLM.generate` of a whole loader batch, thinkdiff/models/
        mllama_vllm_generate_1.py:585 with `max_num_seqs: 256`): any number of requests against `max_live` (default min(256, n_slots)) cache slots.
        A sequence that finishes frees its slot at once -- nothing moves: a decode step names the slot of each of its rows
        (td_qwen2_decode_batch_slots) -- and waiting requests are prefilled into the free slots (one packed pass, td_qwen2_prefill_packed_slots)
        as soon as `admit_min` of them fit (default max_live / 8: a
        prefill pass interrupts the decode steps, so it should be worth a pass), then decode with everybody else.  With outputs of different
        lengths the decode steps stay full, where generate_batch per chunk of max_live runs every chunk down to its longest sequence.
        `request_chunks`: an iterable of request lists -- pulled only when the waiting queue runs low, so a producer (the precompute model's helper
        thread) can build later chunks while earlier ones decode -- or one flat list.  Requests are numbered in arrival order; returns one
        generate()-style dict per request in that order.  forced_output_ids[i]: teacher-forced continuation of request i."""
        forced = forced_output_ids
        max_live = self.max_seqs if max_live is None else int(max_live)
        if max_live < 1 or max_live > self.max_seqs:
            raise _hip.ThinkDiffHipError(f"generate_continuous: max_live={max_live} exceeds min({self.MAX_BATCH}, n_slots={self.n_slots}); call set_slots first")
        admit_min = max(1, max_live // 8) if admit_min is None else max(1, int(admit_min))
        if isinstance(request_chunks, (list, tuple)) and (not request_chunks or isinstance(request_chunks[0], dict)):
            request_chunks = [list(request_chunks)]
            n_known = len(request_chunks[0])
        else:
            n_known = None      # chunks pulled lazily: a per-request list is checked against each chunk as it arrives
        if n_known is not None:
            self._lora_check_call(request_chunks[0])
        sps_req, by_rows = _sampling_list(sampling, n_known, "generate_continuous")
        draft = _draft_source(speculative, "generate_continuous")
        if draft is not None:
            _check_speculative("generate_continuous", [sampling] if sps_req is None else sps_req, forced)
        # n / best_of: request i runs as k_of(i) SEQUENCES, numbered base_of(i) .. in arrival order of their requests (known in advance: one
        # SamplingParams per request, or one for all).  The live rows, `res` and the logprob log are per sequence; the waiting queue and `requests`
        # per request.  Without n / best_of a sequence IS its request.
        if sps_req is None:
            kids1 = sampling.children()
            k_of, base_of, sp_of = (lambda i: len(kids1)), (lambda i: i * len(kids1)), (lambda s: kids1[s % len(kids1)])
            want = kids1[0].logprobs      # (with best_of > n the children are scored though nobody asked)
        else:
            bases = np.concatenate([[0], np.cumsum([sp.width for sp in sps_req])]).tolist()
            seq_sps = [c for sp in sps_req for c in sp.children()]
            k_of, base_of, sp_of = (lambda i: bases[i + 1] - bases[i]), (lambda i: bases[i]), seq_sps.__getitem__
            want = [sp.logprobs for sp in seq_sps] if _LogprobLog.wanted(seq_sps) else None
        wide = [sp for sp in ([sampling] if sps_req is None else sps_req) if sp.width > 1]
        fan = bool(wide)
        if fan and forced is not None:
            raise ValueError("generate_continuous: forced_output_ids with SamplingParams n / best_of > 1: a teacher-forced continuation is one sequence")
        for sp in wide:
            if sp.width > max_live:
                raise _hip.ThinkDiffHipError(f"generate_continuous: SamplingParams n={sp.n}, best_of={sp.best_of} needs {sp.width} cache slots at "
                                             f"once, max_live={max_live}")
        chunk_it = iter(request_chunks)
        requests, res, waiting = [], [], deque()
        exhausted = False

        def pull():
            nonlocal exhausted
            try:
                chunk = next(chunk_it)
            except StopIteration:
                exhausted = True
                return
            for r in chunk:
                n = len(r["prompt_token_ids"])
                if n < 1 or n > min(self.slot_len, self.prefill_rows):
                    raise _hip.ThinkDiffHipError(f"generate_continuous: a prompt of {n} tokens does not fit a slot ({self.slot_len}) / a prefill pass ({self.prefill_rows})")
                if sps_req is not None and len(requests) >= len(sps_req):
                    raise ValueError(f"generate_continuous: {len(sps_req)} SamplingParams for more than {len(sps_req)} requests: pass one SamplingParams, or exactly one per request")
                waiting.append(len(requests))
                requests.append(r)
                for _ in range(k_of(len(requests) - 1)):
                    res.append({"prompt_hidden_states": None, "hidden_states": None, "token_ids": []})

        live = _LiveRows(self, max_live, _TokenSource(self, sampling, by_rows, sp_of, eos_token_id, generator, forced, want, draft), eos_token_id)
        pc = getattr(self, "_prefix_cache", None)
        # (a stack: the lowest free slot is taken first; under prefix caching the cache's allocator, over all n_slots, with max_live bounding the live ones)
        free_slots = list(range(max_live - 1, -1, -1)) if pc is None else _CacheSlots(pc)
        hashes_of = {}      # prefix caching: request -> its block hashes, computed once

        def budget(i):      # tokens (each sequence of) request i may still produce
            return len(forced[i]) if forced is not None else sp_of(base_of(i)).max_tokens

        def fits(free):     # -> (requests, cache slots) of the head of the queue that `free` slots take, in arrival order: nobody overtakes a request that waits for k slots
            if not fan:
                return min(free, len(waiting)), min(free, len(waiting))
            nreq = used = 0
            for i in waiting:
                if used + k_of(i) > free:
                    break
                nreq, used = nreq + 1, used + k_of(i)
            return nreq, used

        while True:
            free = max_live - live.n
            if not exhausted and len(waiting) < free:      # lazily -- the producer builds the next chunk while the current sequences decode -- but enough to fill the free slots
                pull()
                continue
            # ---- admission: one packed prefill pass into free slots (even for a single prompt) ----
            fit, fit_slots = fits(free)
            if fit > 0 and (live.n == 0 or fit_slots >= admit_min or (exhausted and fit >= len(waiting))):
                new, rows, used = [], 0, 0
                # (under prefix caching the pass's rows are counted where it is planned: only the rows behind the cached prefixes are fed)
                while waiting and used + k_of(waiting[0]) <= free and (rows + len(requests[waiting[0]]["prompt_token_ids"]) <= self.prefill_rows
                                                                        or (pc is not None and len(new) < self.MAX_BATCH)):
                    i = waiting.popleft()
                    if budget(i) <= 0:      # nothing to generate: the prompt states only, through the first free slot
                        q = requests[i]
                        e = q.get("inputs_embeds")
                        slot0 = free_slots[-1]
                        self._lora_bind([q], [slot0])
                        res[base_of(i)]["prompt_hidden_states"], _ = self.forward(
                            self._positions(q), torch.tensor(list(q["prompt_token_ids"]), dtype=torch.int32) if e is None else None, e, 0, True, False,
                            slot=slot0)
                        self._lora_release([slot0])
                        continue
                    new.append(i)
                    rows += len(requests[i]["prompt_token_ids"])
                    used += k_of(i)
                if new and pc is not None:      # one pass over as many of them as the cache's plan takes; the rest wait, in order, at the head of the queue
                    qs = [requests[i] for i in new]
                    poss = [self._positions(q) for q in qs]
                    for i, q, p in zip(new, qs, poss):
                        if i not in hashes_of:
                            hashes_of[i] = self._prefix_hashes(q, p)
                    hids, new_slots = self._prefill_pass_cached(pc, qs, poss, [hashes_of[i] for i in new], live.logits[live.n:live.n + len(new)])
                    k = len(new_slots)
                    for i in reversed(new[k:]):
                        waiting.appendleft(i)
                    new, qs, poss = new[:k], qs[:k], poss[:k]
                    for i, h in zip(new, hids):
                        res[base_of(i)]["prompt_hidden_states"] = h
                        hashes_of.pop(i, None)
                    live.admit([base_of(i) for i in new], [k_of(i) for i in new], new_slots, [len(q["prompt_token_ids"]) for q in qs],
                               [int(p.max()) + 1 for p in poss], [budget(i) for i in new], [q["prompt_token_ids"] for q in qs], free_slots)
                    continue
                if new:
                    k, qs = len(new), [requests[i] for i in new]
                    poss = [self._positions(q) for q in qs]
                    emb, pos, lens = self._pack_prompts(qs, poss)
                    hid = torch.empty(rows, self.config.hidden_size, dtype=torch.bfloat16, device=self.device)
                    new_slots = [free_slots.pop() for _ in new]
                    self._lora_bind(qs, new_slots)
                    self._prefill_packed_slots(k, (ctypes.c_int * k)(*new_slots), emb, pos, (ctypes.c_int * k)(*lens), hid, live.logits[live.n:live.n + k])
                    for i, h in zip(new, torch.split(hid, lens)):
                        res[base_of(i)]["prompt_hidden_states"] = h
                    live.admit([base_of(i) for i in new], [k_of(i) for i in new], new_slots, lens, [int(p.max()) + 1 for p in poss],
                               [budget(i) for i in new], [q["prompt_token_ids"] for q in qs], free_slots)
                    continue      # (more may fit in another pass before the next decode step)
            if live.n == 0:
                if waiting or not exhausted:
                    continue
                break
            free_slots.extend(live.step())
        live.results(res)
        return _gather_outputs(res, [sampling] * len(requests) if sps_req is None else sps_req[:len(requests)]) if fan else res

    # the engine calls of generate_continuous (separate methods so that the scheduler's host logic can be exercised against a stand-in engine)
    def _prefill_packed_slots(self, k, slots_c, emb, pos, lens_c, hid_out, logits_out):
        _hip.check(self._L.td_qwen2_prefill_packed_slots(self._h, k, ctypes.cast(slots_c, ctypes.c_void_p), None, _hip.ptr(emb), _hip.ptr(pos),
                                                         ctypes.cast(lens_c, ctypes.c_void_p), _hip.ptr(hid_out), _hip.ptr(logits_out), _hip.stream_ptr()))

    def _prefill_packed_prefix_slots(self, k, slots_c, emb, pos, lens_c, prefix_c, hid_out, logits_out):
        """The packed prefill behind cached prefixes (td_qwen2_prefill_packed_prefix_slots): emb, pos, hid_out cover the lens_c[b] NEW rows of every
        sequence, which go behind the prefix_c[b] rows its slot already holds."""
        _hip.check(self._L.td_qwen2_prefill_packed_prefix_slots(self._h, k, ctypes.cast(slots_c, ctypes.c_void_p), None, _hip.ptr(emb), _hip.ptr(pos),
                                                                ctypes.cast(lens_c, ctypes.c_void_p), ctypes.cast(prefix_c, ctypes.c_void_p), _hip.ptr(hid_out),
                                                                _hip.ptr(logits_out), _hip.stream_ptr()))

    def _prefix_copy(self, src, dst_slots, length):
        """The copy of a cache hit: rows [0, length) of the donor slot to every destination, one launch over all layers (td_qwen2_fork_slot)."""
        dst = (ctypes.c_int * len(dst_slots))(*[int(d) for d in dst_slots])
        _hip.check(self._L.td_qwen2_fork_slot(self._h, int(src), ctypes.cast(dst, ctypes.c_void_p), len(dst_slots), int(length), _hip.stream_ptr()))

    def prefill_packed(self, requests_rows, slots: Sequence[int], prefix_lens: Sequence[int], want_logits=True):
        """The packed prefill behind cached prefixes as a call of its own (tests, callers that keep their own books): requests_rows[b] = dict with
        "position_ids" [3, n_b] and "token_ids" [n_b] or "inputs_embeds" [n_b, hidden] for the n_b NEW rows of sequence b, which go to cache rows
        [prefix_lens[b], prefix_lens[b] + n_b) of slot slots[b]; the caller vouches for the rows in front.  -> ([hidden [n_b, hidden]], logits of each
        sequence's last row [B, vocab] | None).  Drops the prefix cache's entries of the slots it writes."""
        B, D = len(requests_rows), self.config.hidden_size
        if len(slots) != B or len(prefix_lens) != B or B < 1:
            raise _hip.ThinkDiffHipError(f"prefill_packed: {len(slots)} slots and {len(prefix_lens)} prefix_lens for {B} sequences")
        lens = [int(r["position_ids"].shape[1]) for r in requests_rows]
        emb = torch.empty(sum(lens), D, dtype=torch.bfloat16, device=self.device)
        pos = torch.empty(3, sum(lens), dtype=torch.int32)
        r0 = 0
        for r, n in zip(requests_rows, lens):
            e = r.get("inputs_embeds")
            emb[r0:r0 + n] = self.embed_tokens(r["token_ids"]) if e is None else e.to(self.device, torch.bfloat16)
            pos[:, r0:r0 + n] = r["position_ids"].to(torch.int32)
            r0 += n
        hid = torch.empty(sum(lens), D, dtype=torch.bfloat16, device=self.device)
        lg = torch.empty(B, self.config.vocab_size, dtype=torch.bfloat16, device=self.device) if want_logits else None
        self._pc_wrote(slots)
        if getattr(self, "_lora", None) is not None or any(r.get("lora_request") is not None for r in requests_rows):
            self._lora_bind(requests_rows, slots)      # (each dict's "lora_request": the adapter its sequence runs under from here on; none: under none)
        self._prefill_packed_prefix_slots(B, (ctypes.c_int * B)(*[int(s) for s in slots]), emb, pos.to(self.device).contiguous(), (ctypes.c_int * B)(*lens),
                                          (ctypes.c_int * B)(*[int(p) for p in prefix_lens]), hid, lg)
        return list(torch.split(hid, lens)), lg

    # ---- prompt prefill under prefix caching ---------------------------------------------------------------------------------------------------
    def _prefix_hashes(self, request, pos):
        lr = LoRARequest.of(request.get("lora_request"))      # (the same prompt under two adapters shares no block)
        return _pfx.block_hashes(request["prompt_token_ids"], pos, request.get("inputs_embeds"), request.get("mm_hash"), None if lr is None else lr.lora_int_id)

    def _prefill_pass_cached(self, pc, requests, poss, hashes, logits_out):
        """ONE prefill pass over the head of `requests` as the cache plans it (PrefixCache.plan_pass) -> (the prompts' complete hidden states, their cache
        slots) for the first t requests, t >= 1; logits_out[j] receives the last-token logits of request j < t.  All copies of the pass are enqueued in
        front of its prefill; a prompt's hidden states are cat(the donor's first m rows, the new rows)."""
        D = self.config.hidden_size
        lens = [len(q["prompt_token_ids"]) for q in requests]
        stage = self.prefill_rows if getattr(self, "kv_cache_dtype", "auto") == "fp8" else None      # (the e4m3 cache stages prefix + new rows)
        plan = pc.plan_pass(list(zip(hashes, lens)), self.MAX_BATCH, self.prefill_rows, stage)
        t = len(plan)
        if t == 0:
            raise _hip.ThinkDiffHipError("prefix cache: no cache slot left for a waiting request")
        donor_hidden = [None if p.m == 0 else pc.hidden_of(p.donor)[:p.m] for p in plan]      # (before the entries of this pass replace anything)
        for donor, m, dsts in pc.copies(plan):
            self._prefix_copy(donor, dsts, m)
        new = [n - p.m for n, p in zip(lens, plan)]
        emb = torch.empty(sum(new), D, dtype=torch.bfloat16, device=self.device)
        pos = torch.empty(3, sum(new), dtype=torch.int32)
        r = 0
        for q, pp, p, k in zip(requests, poss, plan, new):
            e = q.get("inputs_embeds")
            emb[r:r + k] = self.embed_tokens(q["prompt_token_ids"][p.m:]) if e is None else e[p.m:].to(self.device, torch.bfloat16)
            pos[:, r:r + k] = pp[:, p.m:].to(torch.int32)
            r += k
        hid = torch.empty(sum(new), D, dtype=torch.bfloat16, device=self.device)
        slots = [p.slot for p in plan]
        self._lora_bind(requests[:t], slots)      # (behind the copies: a destination took its donor's adapter, which is the request's own -- the hashes are salted)
        self._prefill_packed_prefix_slots(t, (ctypes.c_int * t)(*slots), emb, pos.to(self.device).contiguous(), (ctypes.c_int * t)(*new),
                                          (ctypes.c_int * t)(*[p.m for p in plan]), hid, logits_out[:t])
        hidden = []
        for h_new, h_old, p, hs in zip(torch.split(hid, new), donor_hidden, plan, hashes):
            h = h_new if h_old is None else torch.cat([h_old, h_new])
            pc.insert(p.slot, hs, h)
            hidden.append(h)
        return hidden, slots

    def _prefill_prompts_cached(self, pc, requests, poss, logits_out):
        """_prefill_prompts under prefix caching -> (the prompts' hidden states, the cache slots the cache chose for them).  Prompts that fit no packed
        pass (or packed_prefill off) go the uncached way into slots from the cache's allocator and leave no entry."""
        B = len(requests)
        lens = [len(q["prompt_token_ids"]) for q in requests]
        if not self.packed_prefill or max(lens) > min(self.slot_len, self.prefill_rows):
            slots = pc.take(B)
            if slots is None:
                raise _hip.ThinkDiffHipError(f"prefix cache: no {B} cache slots left")
            return self._prefill_prompts(requests, slots, poss, logits_out), slots
        hashes = [self._prefix_hashes(q, p) for q, p in zip(requests, poss)]
        hidden, slots, b0 = [], [], 0
        while b0 < B:
            h, s = self._prefill_pass_cached(pc, requests[b0:], poss[b0:], hashes[b0:], logits_out[b0:])
            hidden += h
            slots += s
            b0 += len(s)
        return hidden, slots

    def _decode_slots(self, n, slots_np, tok_dev, pos_dev, cache_np, hid_out, logits_out):
        _hip.check(self._L.td_qwen2_decode_batch_slots(self._h, n, ctypes.c_void_p(slots_np.ctypes.data), _hip.ptr(tok_dev), _hip.ptr(pos_dev),
                                                       ctypes.c_void_p(cache_np.ctypes.data), _hip.ptr(hid_out), _hip.ptr(logits_out), _hip.stream_ptr()))

    def _verify_slots(self, n, slots_np, n_new_np, tok_dev, pos_dev, cache_np, hid_out, logits_out):
        """The verify step of speculative decoding: live row i feeds n_new_np[i] tokens (td_qwen2_verify_batch_slots)."""
        _hip.check(self._L.td_qwen2_verify_batch_slots(self._h, n, ctypes.c_void_p(slots_np.ctypes.data), ctypes.c_void_p(n_new_np.ctypes.data), _hip.ptr(tok_dev),
                                                       _hip.ptr(pos_dev), ctypes.c_void_p(cache_np.ctypes.data), _hip.ptr(hid_out), _hip.ptr(logits_out),
                                                       _hip.stream_ptr()))

    def spec_stats(self) -> dict:
        """Of the last call with speculative=: steps (passes over the weights), drafted (guesses fed), accepted (guesses that matched the sampled
        token), emitted (tokens the sequences advanced by).  Empty before the first such call."""
        return dict(getattr(self, "_spec_stats", {}))

    def _fork_slots(self, src, dst_slots, length):
        """The fork of n / best_of admission: the `length` prompt rows of slot `src` to every slot of dst_slots (a method of its own beside the two
        above, for the same reason)."""
        self.fork_slot(src, dst_slots, length)

    def fork_slot(self, src: int, dst_slots: Sequence[int], length: int):
        """Copy the first `length` cache rows of slot `src` to every slot of `dst_slots` in ONE launch over all layers (td_qwen2_fork_slot: each source
        chunk is read once and written len(dst_slots) times): the sequences in those slots then continue from the same prefill."""
        dst = (ctypes.c_int * max(1, len(dst_slots)))(*[int(d) for d in dst_slots])
        self._pc_wrote(dst_slots)
        _hip.check(self._L.td_qwen2_fork_slot(self._h, int(src), ctypes.cast(dst, ctypes.c_void_p), len(dst_slots), int(length), _hip.stream_ptr()))
        self._lora_inherit(src, dst_slots)      # (the device map did the same inside the call)

    def gather_slots(self, slots: Sequence[int], copy_src, lengths: Sequence[int]):
        """For every row j with copy_src[j] >= 0 (an int32 DEVICE tensor, read by the kernel: the host never learns it), copy the first lengths[j]
        cache rows of slot slots[copy_src[j]] to slot slots[j], all layers and planes (td_qwen2_gather_slots).  The caller vouches that no
        destination is a source of the same call -- beam_select's placement guarantees it."""
        n = len(slots)
        sl = (ctypes.c_int * max(1, n))(*[int(v) for v in slots])
        ln = (ctypes.c_int * max(1, n))(*[int(v) for v in lengths])
        src = copy_src.to(device=self.device, dtype=torch.int32).contiguous()
        if src.numel() != n or len(lengths) != n:
            raise _hip.ThinkDiffHipError(f"gather_slots: {src.numel()} copy_src entries and {len(lengths)} lengths for {n} slots")
        self._pc_wrote(slots)
        _hip.check(self._L.td_qwen2_gather_slots(self._h, n, ctypes.cast(sl, ctypes.c_void_p), _hip.ptr(src), ctypes.cast(ln, ctypes.c_void_p), _hip.stream_ptr()))

    # ---- prompt prefill of generate_batch, generate_continuous and beam_search ---------------------------------------------------------------
    def _positions(self, request):
        p = request.get("position_ids")
        return self.text_position_ids(len(request["prompt_token_ids"])) if p is None else p

    def _pack_prompts(self, requests, poss):
        """The prompts back to back, no padding rows -> (emb bf16 [rows, hidden] and pos int32 [3, rows] on the device, the prompts' lengths)."""
        lens = [len(q["prompt_token_ids"]) for q in requests]
        emb = torch.empty(sum(lens), self.config.hidden_size, dtype=torch.bfloat16, device=self.device)
        pos = torch.empty(3, sum(lens), dtype=torch.int32)
        r = 0
        for q, pp, n in zip(requests, poss, lens):
            e = q.get("inputs_embeds")
            emb[r:r + n] = self.embed_tokens(q["prompt_token_ids"]) if e is None else e.to(self.device, torch.bfloat16)
            pos[:, r:r + n] = pp.to(torch.int32)
            r += n
        return emb, pos.to(self.device).contiguous(), lens

    def _prefill_prompts(self, requests, slots, poss, logits_out, padded_ok=False):
        """Prompt j into cache slot slots[j], its last token's logits into logits_out[j] -> the prompts' hidden states, one tensor per request.
        Several prompts that each fit a pass are packed (packed_prefill: td_qwen2_prefill_packed_slots -- vLLM's batching of the reference's
        requests), a pass taking as many prompts as the activation workspace (max_num_batched_tokens) and MAX_BATCH hold; with packed_prefill off
        and padded_ok (generate_batch alone: slots must be consecutive) they are right-padded to the longest (td_qwen2_prefill_batch_at: A/B,
        tests); anything else is one forward per prompt."""
        B, D = len(requests), self.config.hidden_size
        lens = [len(q["prompt_token_ids"]) for q in requests]
        hidden = [None] * B
        L = (max(lens) + 7) // 8 * 8
        self._lora_bind(requests, slots)
        if B > 1 and self.packed_prefill and max(lens) <= min(self.slot_len, self.prefill_rows):
            b0 = 0
            while b0 < B:
                nb, rows = 0, 0
                while b0 + nb < B and nb < self.MAX_BATCH and rows + lens[b0 + nb] <= self.prefill_rows:
                    rows += lens[b0 + nb]
                    nb += 1
                emb, pos, ln = self._pack_prompts(requests[b0:b0 + nb], poss[b0:b0 + nb])
                hid = torch.empty(rows, D, dtype=torch.bfloat16, device=self.device)
                self._prefill_packed_slots(nb, (ctypes.c_int * nb)(*slots[b0:b0 + nb]), emb, pos, (ctypes.c_int * nb)(*ln), hid, logits_out[b0:b0 + nb])
                hidden[b0:b0 + nb] = torch.split(hid, ln)
                b0 += nb
        elif padded_ok and B > 1 and L <= self.slot_len and 2 * L <= self.prefill_rows:
            # one pass over the weights for as many prompts as the activation workspace holds (all of them, normally): right-padded
            # to L rows each (causal attention keeps the padding inert); a larger request batch takes several such passes
            per = min(B, self.prefill_rows // L)
            for b0 in range(0, B, per):
                nb = min(per, B - b0)
                emb = torch.zeros(nb * L, D, dtype=torch.bfloat16, device=self.device)
                pos = torch.zeros(3, nb * L, dtype=torch.int32)
                for j in range(nb):
                    q, n, p = requests[b0 + j], lens[b0 + j], poss[b0 + j]
                    e = q.get("inputs_embeds")
                    emb[j * L:j * L + n] = self.embed_tokens(q["prompt_token_ids"]) if e is None else e.to(self.device, torch.bfloat16)
                    pos[:, j * L:j * L + n] = p.to(torch.int32)
                    pos[:, j * L + n:(j + 1) * L] = int(p.max()) + 1 + torch.arange(L - n, dtype=torch.int32)
                pos = pos.to(self.device).contiguous()
                hid = torch.empty(nb * L, D, dtype=torch.bfloat16, device=self.device)
                cl = (ctypes.c_int * nb)(*lens[b0:b0 + nb])
                _hip.check(self._L.td_qwen2_prefill_batch_at(self._h, slots[b0], nb, L, None, _hip.ptr(emb), _hip.ptr(pos), ctypes.cast(cl, ctypes.c_void_p),
                                                             _hip.ptr(hid), _hip.ptr(logits_out[b0:b0 + nb]), _hip.stream_ptr()))
                for j in range(nb):
                    hidden[b0 + j] = hid[j * L:j * L + lens[b0 + j]]
        else:
            for j, (q, p) in enumerate(zip(requests, poss)):
                e = q.get("inputs_embeds")
                hidden[j], lg = self.forward(p, torch.tensor(list(q["prompt_token_ids"]), dtype=torch.int32) if e is None else None, e, 0, True, True, slot=slots[j])
                logits_out[j] = lg
        return hidden

    # ---- beam search ([ext] vllm.LLM.beam_search) ------------------------------------------------------------------------------------------
    @_prefix_entry
    @torch.no_grad()
    def beam_search(self, requests: Sequence[dict], params: BeamSearchParams, eos_token_id: Optional[int] = None):
        """vLLM's `LLM.beam_search` for R requests (the dicts of generate_batch) with W = params.beam_width beams each, on R x W cache slots: request r
        owns slots r W .. r W + W - 1 and is prefilled once, into the first.  Then T = max_tokens rounds of

            logprobs_rows(2 W) -> beam_select -> gather_slots -> decode step (device tokens, fixed slots, host-known cache lengths)

        are ENQUEUED without a synchronisation: the choice of the next beams, their placement and the reordering of the cache rows all happen on
        the device (td_beam_select, td_kv_gather_rows; the first round's gather is the fork of the prompt), and the per-step logs [T, R W] are read
        once after the loop.  The host then walks the `parent` chains.

        A candidate equal to EOS (eos_token_id, unless ignore_eos) completes a sequence instead of becoming a beam: a finisher logged at round s is
        s + 1 tokens ending in EOS, with hidden states for the s tokens before it -- the EOS is never fed to the decoder.  Per request the completed
        sequences (in creation order) and then the live beams (by rank) are sorted stably by score = cum / seq_len ** length_penalty, descending,
        where seq_len = prompt length + generated tokens, less one if the last token is EOS; the first W are returned.

        -> per request a dict with generate()'s keys for output 0 ("prompt_hidden_states", "hidden_states", "token_ids"), "cumulative_logprob", "score"
        and "outputs": W dicts with "index", "token_ids", "hidden_states", "cumulative_logprob", "score", "finished"."""
        params.validate()
        R, W, T = len(requests), int(params.beam_width), int(params.max_tokens)
        if R < 1:
            raise ValueError("beam_search: no requests")
        self._lora_check_call(requests)
        if R * W > self.max_seqs:
            raise _hip.ThinkDiffHipError(f"beam_search: {R} requests x beam_width={W} need {R * W} cache slots, which exceed min({self.MAX_BATCH}, n_slots={self.n_slots}); "
                                         "call set_slots first")
        plen = [len(r["prompt_token_ids"]) for r in requests]
        for i, n in enumerate(plen):
            if n < 1:
                raise ValueError(f"beam_search: request {i} has an empty prompt")
            if n + T > self.slot_len:
                raise _hip.ThinkDiffHipError(f"beam_search: request {i}: prompt length {n} + max_tokens={T} exceeds the slot capacity {self.slot_len}")
        V, D = self.config.vocab_size, self.config.hidden_size
        if V <= 2 * W:
            raise ValueError(f"beam_search: vocab_size={V} must exceed 2 x beam_width = {2 * W}: a step takes the 2 x beam_width most probable tokens of a row")
        if eos_token_id is not None and not 0 <= int(eos_token_id) < V:
            raise ValueError(f"beam_search: eos_token_id={eos_token_id} outside the vocabulary of {V}")
        eos = -1 if (params.ignore_eos or eos_token_id is None) else int(eos_token_id)
        N, dev = R * W, self.device
        poss = [self._positions(r) for r in requests]
        next_pos = [int(p.max()) + 1 for p in poss]
        logits0 = torch.empty(R, V, dtype=torch.bfloat16, device=dev)
        pc = getattr(self, "_prefix_cache", None)
        slots_np = np.arange(N, dtype=np.int32)
        if pc is None:
            prompt_hidden = self._prefill_prompts(requests, [r * W for r in range(R)], poss, logits0)      # each prompt once, into its request's first slot
        else:      # prefix caching: the cache places the prompts; the other beams of a request take slots from its allocator
            prompt_hidden, parents = self._prefill_prompts_cached(pc, requests, poss, logits0)
            kids = pc.take(N - R) if N > R else []
            if kids is None:
                raise _hip.ThinkDiffHipError(f"beam_search: the prefix cache has no {N - R} cache slots left for the beams")
            for r in range(R):
                slots_np[r * W:(r + 1) * W] = [parents[r]] + kids[r * (W - 1):(r + 1) * (W - 1)]
        # per-request LoRA: the gather cannot know its source rows, so every beam slot of a request is set to the request's adapter once, here
        if getattr(self, "_lora", None) is not None:
            self._lora_bind([requests[r] for r in range(R) for _ in range(W)], slots_np)
        # what the loop needs from the host, uploaded before it starts: the rows' M-RoPE positions of every round and the first round's live rows
        first = torch.arange(R, dtype=torch.int64) * W
        logits = torch.zeros(N, V, dtype=torch.bfloat16, device=dev)
        logits[first.to(dev)] = logits0
        pos_all = (torch.tensor(next_pos, dtype=torch.int32).repeat_interleave(W)[None, None, :] + torch.arange(T, dtype=torch.int32)[:, None, None]) \
            .expand(T, 3, N).contiguous().to(dev)
        n_top0 = torch.full((N,), -1, dtype=torch.int32)
        n_top0[first] = 2 * W
        n_top0, n_top = n_top0.to(dev), torch.full((N,), 2 * W, dtype=torch.int32).to(dev)
        no_ids = torch.zeros(N, dtype=torch.int32, device=dev)      # (td_logprobs_rows_bf16 also scores a chosen token per row: unused here)
        ilog = torch.empty(5, T, N, dtype=torch.int32, device=dev)      # token, rank, copy_src, parent, fin_flag
        flog = torch.empty(2, T, N, dtype=torch.float32, device=dev)    # cum, fin_cum
        cum0, rank0 = torch.zeros(N, dtype=torch.float32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
        hid_all = torch.empty(T, N, D, dtype=torch.bfloat16, device=dev)
        base_len = np.repeat(np.asarray(plen, dtype=np.int32), W)
        for s in range(T):
            _, _, top_ids, top_lp = _OPS.logprobs_rows(logits, no_ids, n_top0 if s == 0 else n_top, 2 * W)
            _OPS.beam_select(top_ids, top_lp, cum0 if s == 0 else flog[0, s - 1], rank0 if s == 0 else ilog[1, s - 1], W, 1 if s == 0 else W, eos,
                             ilog[0, s], flog[0, s], ilog[1, s], ilog[2, s], ilog[3, s], ilog[4, s], flog[1, s])
            cache_np = base_len + np.int32(s)
            self.gather_slots(slots_np, ilog[2, s], cache_np)
            # every row decodes: vocab > 2 W leaves each live row at least 2 W - 1 >= W candidates that are not EOS, so no beam is ever missing (token -1)
            self._decode_slots(N, slots_np, ilog[0, s], pos_all[s], cache_np, hid_all[s], logits)
        ilog_h, flog_h = ilog.cpu().numpy(), flog.cpu().numpy()      # the one download
        tok_l, rank_l, par_l, fin_l, cum_l, fcum_l = ilog_h[0], ilog_h[1], ilog_h[3], ilog_h[4], flog_h[0], flog_h[1]

        def chain(s, row):
            """The tokens of the beam living in `row` after round s, and where their hidden rows lie in hid_all.view(T N, D)."""
            toks, idx = [], []
            while s >= 0:
                toks.append(int(tok_l[s, row]))
                idx.append(s * N + row)
                row, s = int(par_l[s, row]), s - 1
            return toks[::-1], idx[::-1]

        results, picks = [], []
        for r in range(R):
            seqs = []      # (tokens, hidden rows, cum, finished): completed sequences in creation order, then the live beams by rank
            for s in range(T):
                rows = [r * W] if s == 0 else sorted(range(r * W, r * W + W), key=lambda q: int(rank_l[s - 1, q]))
                for q in rows:
                    if fin_l[s, q]:
                        toks, idx = chain(s - 1, q) if s else ([], [])
                        seqs.append((toks + [eos], idx, float(fcum_l[s, q]), True))
            for q in sorted(range(r * W, r * W + W), key=lambda q: int(rank_l[T - 1, q])):
                toks, idx = chain(T - 1, q)
                seqs.append((toks, idx, float(cum_l[T - 1, q]), False))
            scored = [(params.score(c, plen[r] + len(t) - (1 if eos_token_id is not None and t[-1] == int(eos_token_id) else 0)), t, i, c, f) for t, i, c, f in seqs]
            scored.sort(key=lambda x: -x[0])      # (stable: ties keep the order above)
            picks.append(scored[:W])
        flat = [i for pk in picks for _, _, idx, _, _ in pk for i in idx]
        parts = iter(torch.split(hid_all.view(T * N, D).index_select(0, torch.tensor(flat, dtype=torch.int64).to(dev)),
                                 [len(idx) for pk in picks for _, _, idx, _, _ in pk]))
        for r, pk in enumerate(picks):
            outs = [{"index": k, "token_ids": t, "hidden_states": next(parts), "cumulative_logprob": c, "score": sc, "finished": f}
                    for k, (sc, t, _, c, f) in enumerate(pk)]
            results.append({"prompt_hidden_states": prompt_hidden[r], "hidden_states": outs[0]["hidden_states"], "token_ids": outs[0]["token_ids"],
                            "cumulative_logprob": outs[0]["cumulative_logprob"], "score": outs[0]["score"], "outputs": outs})
        return results

    def move_slot(self, src: int, dst: int, length: int):
        """Copy the first `length` cache rows of slot `src` to slot `dst` (td_qwen2_move_slot).  The decode steps name their slots, so nothing in this
        class needs it any more; it stays for callers that want to defragment a handle before re-partitioning it (set_slots)."""
        self._pc_wrote([dst])
        _hip.check(self._L.td_qwen2_move_slot(self._h, int(src), int(dst), int(length), _hip.stream_ptr()))
        self._lora_inherit(src, [dst])


def smart_resize(height: int, width: int, factor: int = 28, min_pixels: int = 4 * 28 * 28, max_pixels: int = 16384 * 28 * 28):
    """[ext] qwen_vl_utils.smart_resize / transformers Qwen2-VL image processing: both sides to multiples of `factor`,
    area inside [min_pixels, max_pixels], aspect ratio kept as closely as the grid allows."""
    import math
    if max(height, width) / min(height, width) > 200:
        raise ValueError(f"absolute aspect ratio must be smaller than 200, got {max(height, width) / min(height, width)}")
    h_bar = max(factor, round(height / factor) * factor)
    w_bar = max(factor, round(width / factor) * factor)
    if h_bar * w_bar > max_pixels:
        beta = math.sqrt((height * width) / max_pixels)
        h_bar = max(factor, math.floor(height / beta / factor) * factor)
        w_bar = max(factor, math.floor(width / beta / factor) * factor)
    elif h_bar * w_bar < min_pixels:
        beta = math.sqrt(min_pixels / (height * width))
        h_bar = math.ceil(height * beta / factor) * factor
        w_bar = math.ceil(width * beta / factor) * factor
    return h_bar, w_bar


def process_vision_info(conversations):
    """The image half of [ext] qwen_vl_utils.process_vision_info, which the reference's multi-image drivers call on their
    chat messages (scripts/test/test_mllama_t5_decoder_flux_multi_image.py:223): every {"type": "image", "image": path | PIL,
    ["min_pixels", "max_pixels" | "resized_height", "resized_width"]} part, in message order, opened as RGB and resized
    so that both sides are multiples of 28 and the area lies inside the part's pixel budget (defaults 4*28*28 ..
    16384*28*28).  Returns (images | None, None) -- videos are not part of the ThinkDiff path."""
    from PIL import Image
    convs = conversations if conversations and isinstance(conversations[0], (list, tuple)) else [conversations]
    images = []
    for conv in convs:
        for turn in conv:
            if isinstance(turn.get("content"), str):
                continue
            for part in turn["content"]:
                if part.get("type") != "image" and "image" not in part:
                    continue
                im = part["image"]
                if isinstance(im, str):
                    im = Image.open(im[len("file://"):] if im.startswith("file://") else im)
                im = im.convert("RGB")
                if "resized_height" in part and "resized_width" in part:
                    rh, rw = smart_resize(part["resized_height"], part["resized_width"], factor=28)
                else:
                    w, h = im.size
                    rh, rw = smart_resize(h, w, factor=28, min_pixels=part.get("min_pixels", 4 * 28 * 28),
                                          max_pixels=part.get("max_pixels", 16384 * 28 * 28))
                images.append(im.resize((rw, rh)))
    return (images or None), None


SYSTEM_PROMPT = "You are a helpful assistant."   # reference mllama_vllm_t5_embed_decoder_2.py:1048, mllama_vllm_generate_1.py:551


class QwenChatFrontend:
    """What vLLM's Qwen2-VL input pipeline does around the decoder, shared by the two LVLM model mirrors: ChatML request
    building, tokenisation, the vision tower, placeholder expansion / embedding splice and M-RoPE positions.
    Expects on `self`: mllama (Qwen2VLTextEngine), mllama_processor, mllama_tokenizer, image_processor, visual, image_token_id."""

    mllama_lora_request = None      # vllm_config["lora_request"]: the one adapter every request of the model class runs under

    def with_lora_request(self, reqs: Sequence[dict]) -> List[dict]:
        """The requests under the model's adapter (a request that names one of its own keeps it); with none configured: the requests as they are."""
        if self.mllama_lora_request is None:
            return list(reqs)
        return [r if r.get("lora_request") is not None else dict(r, lora_request=self.mllama_lora_request) for r in reqs]

    def chat_requests(self, texts, images) -> List[dict]:
        """(instruction, [image]) pairs -> [{"prompt", "multi_modal_data": {"image": ...}}] exactly as the reference builds
        them (system turn + user turn with one image part then the text part, generation prompt appended)."""
        if self.mllama_processor is None:
            raise _hip.ThinkDiffHipError(
                "text requests need the Qwen2-VL processor / chat template loaded from a local path (or the synthetic stand-in); "
                "pass need_process=False with {'prompt_token_ids': ...} requests instead")
        msgs = [[{"role": "system", "content": SYSTEM_PROMPT},
                 {"role": "user", "content": ([{"type": "image", "image": im}] if im is not None else []) + [{"type": "text", "text": t}]}]
                for t, im in zip(texts, images)]
        prompts = self.mllama_processor.apply_chat_template(msgs, tokenize=False, add_generation_prompt=True)
        return [{"prompt": p, "multi_modal_data": {"image": im}} for p, im in zip(prompts, images)]

    def splice_images(self, ids, images):
        """Prompt ids with one placeholder per image -> (expanded ids, inputs_embeds [n, hidden], position_ids [3, n])."""
        if self.visual is None or self.image_processor is None:
            raise _hip.ThinkDiffHipError("image request: load the vision tower (visual=HipQwen2VisionTransformer...) and an "
                                         "image_processor, or supply 'inputs_embeds' and 'position_ids' with the request")
        images = list(images) if isinstance(images, (list, tuple)) else [images]
        feats = self._preprocess_on_device(images) or self.image_processor(images=images, return_tensors="pt")
        grid = feats["image_grid_thw"].tolist() if torch.is_tensor(feats["image_grid_thw"]) else feats["image_grid_thw"]
        merged = self.visual(feats["pixel_values"], grid).pooler_output
        merge = self.visual.merge
        ids = Qwen2VLTextEngine.expand_image_placeholders(ids, grid, merge, self.image_token_id)
        emb = self.mllama.embed_tokens(ids)
        mask = torch.tensor(ids) == self.image_token_id
        emb[mask.to(emb.device)] = merged
        return ids, emb, Qwen2VLTextEngine.mrope_position_ids(ids, grid, merge, self.image_token_id)

    def resolve_requests(self, reqs: Sequence[dict]) -> List[dict]:
        """resolve_request for a batch: all images of the batch go through the image processor and the vision tower in ONE
        call (the tower's GEMMs then see thousands of patch rows instead of one image's few hundred)."""
        out = [dict(r) for r in reqs]
        for r in out:
            if "prompt_token_ids" not in r:
                if self.mllama_tokenizer is None:
                    raise _hip.ThinkDiffHipError("request has no 'prompt_token_ids' and no tokenizer is loaded")
                r["prompt_token_ids"] = self.mllama_tokenizer.encode(r["prompt"], add_special_tokens=False)
        need = [i for i, r in enumerate(out) if (r.get("multi_modal_data") or {}).get("image") is not None and "inputs_embeds" not in r]
        if not need:
            return out
        if self.visual is None or self.image_processor is None:
            raise _hip.ThinkDiffHipError("image request: load the vision tower (visual=HipQwen2VisionTransformer...) and an "
                                         "image_processor, or supply 'inputs_embeds' and 'position_ids' with the request")
        per_req = []
        for i in need:
            im = out[i]["multi_modal_data"]["image"]
            per_req.append(list(im) if isinstance(im, (list, tuple)) else [im])
        flat = [im for ims in per_req for im in ims]
        feats = self._preprocess_on_device(flat)
        if feats is None and len(flat) > 2:      # resize / normalise / patchify is CPU work per image: spread it over threads (PIL and numpy drop the GIL)
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(8, len(flat))) as pool:
                parts = list(pool.map(lambda im: self.image_processor(images=[im], return_tensors="pt"), flat))
            feats = {"pixel_values": torch.cat([f["pixel_values"] for f in parts]), "image_grid_thw": torch.cat([f["image_grid_thw"] for f in parts])}
        elif feats is None:
            feats = self.image_processor(images=flat, return_tensors="pt")
        grid = feats["image_grid_thw"].tolist() if torch.is_tensor(feats["image_grid_thw"]) else feats["image_grid_thw"]
        merged = self.visual(feats["pixel_values"], grid).pooler_output
        merge = self.visual.merge
        counts = [t * h * w // (merge * merge) for t, h, w in grid]
        # One embedding gather and ONE scatter of the merged vision tokens for the whole batch: the placeholder positions are known on
        # the host (they are token ids), so nothing here waits for the device -- a boolean-mask assignment per request would
        # synchronise with the vision tower once per request.
        g0 = 0
        all_ids, spans, grids = [], [], []
        for i, ims in zip(need, per_req):
            g = grid[g0:g0 + len(ims)]
            ids = Qwen2VLTextEngine.expand_image_placeholders(list(out[i]["prompt_token_ids"]), g, merge, self.image_token_id)
            spans.append((len(all_ids), len(all_ids) + len(ids)))
            all_ids += ids
            grids.append(g)
            g0 += len(ims)
        flat_ids = np.asarray(all_ids, dtype=np.int64)
        where = np.flatnonzero(flat_ids == self.image_token_id)
        if where.size != sum(counts):
            raise ValueError(f"the batch holds {where.size} image placeholder tokens for {sum(counts)} merged vision tokens")
        emb_all = self.mllama.embed_tokens(all_ids)
        emb_all.index_copy_(0, torch.from_numpy(where).to(emb_all.device), merged.to(emb_all.dtype))
        for i, (a0, a1), g in zip(need, spans, grids):
            r = out[i]
            ids = all_ids[a0:a1]
            r["prompt_token_ids"], r["inputs_embeds"] = ids, emb_all[a0:a1]
            r["position_ids"] = Qwen2VLTextEngine.mrope_position_ids(ids, g, merge, self.image_token_id)
        for i, ims in zip(need, per_req):
            self._fill_mm_hash(out[i], ims)
        return out

    def _device_preprocess_plan(self):
        """Settings of the image processor when its pipeline is the PIL one of transformers (convert to RGB, smart_resize +
        PIL resize, rescale, normalize, patchify) -- then the whole of it runs on the device: the resize with the RGB conversion of
        "L" / "RGBA" folded in (td_image_resize_u8, Pillow's bytes) and the rest as one more launch per image
        (td_qwen2_patchify_u8).  A `resample` other than LANCZOS / BILINEAR / BICUBIC keeps the resize on the host in PIL.
        None for any other processor: it is called as is."""
        ip = self.image_processor
        plan = getattr(self, "_dev_pre_plan", None)
        if plan is not None and plan[0] is ip:
            return plan[1]
        out = None
        try:
            if type(ip).__name__ == "Qwen2VLImageProcessorPil" and hasattr(self.visual, "padded_patch_dim"):
                ramp = np.arange(256, dtype=np.uint8)[None, None, :].repeat(3, 0)          # [C, 1, 256] channels first, as the backend holds images
                x = ip.rescale(ramp, ip.rescale_factor) if ip.do_rescale else ramp
                x = ip.normalize(x, ip.image_mean, ip.image_std) if ip.do_normalize else x
                lut = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(3, 256))).to(self.visual.device)
                size = ip.size
                out = dict(lut=lut, patch=int(ip.patch_size), merge=int(ip.merge_size), temporal=int(ip.temporal_patch_size), resample=int(ip.resample),
                           do_resize=bool(ip.do_resize), convert_rgb=bool(ip.do_convert_rgb), min_pixels=int(size["shortest_edge"]), max_pixels=int(size["longest_edge"]))
                if 3 * out["temporal"] * out["patch"] ** 2 > self.visual.padded_patch_dim or out["merge"] != self.visual.merge:
                    out = None
        except Exception:
            out = None
        self._dev_pre_plan = (ip, out)
        return out

    def _preprocess_on_device(self, images):
        """PIL images -> {"pixel_values": bf16 [S, Kpad] on the device, "image_grid_thw": [[1, gh, gw], ...]} or None (caller falls back
        to the processor).  Host: the image's bytes as a uint8 array in its own mode ("L", "RGB", "RGBA"; any other mode through
        convert("RGB")) and smart_resize's arithmetic; device: RGB conversion + resize, then rescale / normalize / patchify."""
        plan = self._device_preprocess_plan()
        from PIL import Image
        if plan is None or not images or not all(isinstance(im, Image.Image) for im in images):
            return None
        if not plan["convert_rgb"] and any(im.mode != "RGB" for im in images):
            return None
        f = plan["patch"] * plan["merge"]
        device_resize = plan["resample"] in (1, 2, 3)       # Pillow's LANCZOS, BILINEAR, BICUBIC: the filters td_resize_coeffs builds

        def target(h, w):
            if plan["do_resize"]:
                return smart_resize(h, w, factor=f, min_pixels=plan["min_pixels"], max_pixels=plan["max_pixels"])
            if h % f or w % f:
                raise ValueError(f"image {w}x{h} is not a multiple of {f} and the processor does not resize")
            return h, w

        def prep(im):
            if device_resize:
                im = im if im.mode in ("L", "RGB", "RGBA") else im.convert("RGB")
                a = np.ascontiguousarray(np.asarray(im, dtype=np.uint8))
                return a[:, :, None] if a.ndim == 2 else a
            im = im.convert("RGB") if im.mode != "RGB" else im
            w, h = im.size
            h2, w2 = target(h, w)
            if (h2, w2) != (h, w):
                im = im.resize((w2, h2), resample=plan["resample"])
            return np.ascontiguousarray(np.asarray(im, dtype=np.uint8))

        if len(images) > 2:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(16, len(images))) as pool:
                arrs = list(pool.map(prep, images))
        else:
            arrs = [prep(im) for im in images]
        p = plan["patch"]
        sizes = [target(a.shape[0], a.shape[1]) if device_resize else a.shape[:2] for a in arrs]
        grid = [[1, h // p, w // p] for h, w in sizes]
        Kpad = self.visual.padded_patch_dim
        dev = self.visual.device
        out = torch.empty(sum(g[1] * g[2] for g in grid), Kpad, dtype=torch.bfloat16, device=dev)
        r0 = 0
        for a, g, (h2, w2) in zip(arrs, grid, sizes):
            n = g[1] * g[2]
            img = torch.from_numpy(a).to(dev)
            if a.shape != (h2, w2, 3):
                img = _hip.image_resize_u8(img, h2, w2, plan["resample"], out_channels=3)
            _hip.qwen2_patchify_u8(img, plan["lut"], p, plan["merge"], plan["temporal"], Kpad, out=out[r0:r0 + n])
            r0 += n
        return {"pixel_values": out, "image_grid_thw": grid}

    def resolve_request(self, r: dict) -> dict:
        """Fill prompt_token_ids (tokenizer) and, for image requests, inputs_embeds + position_ids."""
        r = dict(r)
        if "prompt_token_ids" not in r:
            if self.mllama_tokenizer is None:
                raise _hip.ThinkDiffHipError("request has no 'prompt_token_ids' and no tokenizer is loaded")
            r["prompt_token_ids"] = self.mllama_tokenizer.encode(r["prompt"], add_special_tokens=False)
        mm = r.get("multi_modal_data") or {}
        if mm.get("image") is not None and "inputs_embeds" not in r:
            r["prompt_token_ids"], r["inputs_embeds"], r["position_ids"] = self.splice_images(list(r["prompt_token_ids"]), mm["image"])
            self._fill_mm_hash(r, mm["image"])
        return r

    def _fill_mm_hash(self, r: dict, images):
        """While prefix caching is on, an image request carries "mm_hash" (vLLM's multimodal hash), here a digest of the image bytes on the host: the identity
        of its embedding rows in the cache's keys, so that a lookup costs no device read-back.  A hash the request brought is kept."""
        if getattr(getattr(self, "mllama", None), "_prefix_cache", None) is not None and r.get("mm_hash") is None:
            r["mm_hash"] = _pfx.image_digest(images)
