"""Per-request LoRA for the Qwen2-VL decode engine ([ext] vLLM `enable_lora` with a `LoRARequest` per request): the host side.

The engine keeps UNMERGED adapters: every row of a prefill or a decode step names its own adapter and td_lora_rows_bf16 (csrc/lora_rows.hip) adds
`scale * lora_B(lora_A(x))` behind each of the 7 Linears of a decoder layer, so requests under different adapters share one pass over the base weights.
Here: vLLM's `LoRARequest`, the `vllm_config` keys, the loader for peft's published layout and the pool's bookkeeping (which adapter sits at which of the
engine's max_loras places, which cache slot runs under which adapter, whom to drop when the pool is full).  This module knows no engine:
Qwen2VLTextEngine carries its decisions out (tests/test_qwen2_lora_cpu.py runs it on a stand-in).

Loader.  A peft directory (`adapter_config.json` + `adapter_model.safetensors`) or a state dict plus a config dict.  Keys are
`base_model.model.` + `model.layers.N.<module>.lora_A.weight` / `.lora_B.weight`, with an optional `language_model.` component in either published position
(`model.language_model.layers.N...` or `language_model.model.layers.N...`), an optional adapter name (`.lora_A.default.weight`) and an optional leading
`base_model.model.`.  Tensors of another float dtype are rounded to bf16 ONCE, at load.  Honoured: `r`, `lora_alpha`, `use_rslora`
(scale = lora_alpha / r, or lora_alpha / sqrt(r)).  Everything else that would change the model is refused by name, never ignored.
"""
import collections
import dataclasses
import json
import math
import os
import re
from typing import Dict, List, Optional, Tuple

import torch

MODULES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
MAX_LORAS = 8        # TD_LORA_MAX_ADAPTERS
MAX_RANK = 64        # TD_LORA_ROWS_MAX_RANK


@dataclasses.dataclass(frozen=True)
class LoRARequest:
    """vLLM's `LoRARequest`: a name, a positive integer id that identifies the adapter (two requests with one id are one adapter) and where it lies on disk
    (None: it must have been given to `add_lora` with its tensors)."""
    lora_name: str
    lora_int_id: int
    lora_path: Optional[str] = None

    def __post_init__(self):
        if isinstance(self.lora_int_id, bool) or not isinstance(self.lora_int_id, int) or self.lora_int_id < 1:
            raise ValueError(f"LoRARequest: lora_int_id={self.lora_int_id!r} must be an integer >= 1")

    @classmethod
    def of(cls, value) -> Optional["LoRARequest"]:
        """None, a LoRARequest, or a dict of its three fields (the `vllm_config` spelling)."""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, dict):
            extra = set(value) - {"lora_name", "lora_int_id", "lora_path"}
            if extra or "lora_name" not in value or "lora_int_id" not in value:
                raise ValueError(f"lora_request={value!r}: a dict of lora_name, lora_int_id and (optionally) lora_path")
            return cls(value["lora_name"], value["lora_int_id"], value.get("lora_path"))
        raise ValueError(f"lora_request={value!r} is neither a LoRARequest nor a dict of its fields")


def lora_fields_from_vllm_config(vc) -> dict:
    """The LoRA keys of a `vllm_config` as the model classes take them -> dict(enable_lora, max_loras, max_lora_rank, lora_request).  Keys vLLM has and the
    engine does not serve are a ValueError naming the key, never ignored."""
    vc = vc or {}
    if vc.get("fully_sharded_loras"):
        raise ValueError("vllm_config fully_sharded_loras is not served by the HIP engine: one device holds every adapter whole")
    if vc.get("lora_extra_vocab_size"):
        raise ValueError(f"vllm_config lora_extra_vocab_size={vc['lora_extra_vocab_size']!r} is not served by the HIP engine: adapters never touch the embeddings or lm_head")
    if vc.get("long_lora_scaling_factors") is not None:
        raise ValueError("vllm_config long_lora_scaling_factors is not served by the HIP engine")
    if vc.get("lora_dtype", "auto") not in ("auto", "bfloat16"):
        raise ValueError(f"vllm_config lora_dtype={vc['lora_dtype']!r} is not served by the HIP engine: adapters are held in bf16 ('auto' / 'bfloat16')")
    enable = vc.get("enable_lora", False)
    if not isinstance(enable, bool):
        raise ValueError(f"vllm_config enable_lora={enable!r} must be True or False")
    out = {"enable_lora": enable, "max_loras": vc.get("max_loras", 1), "max_lora_rank": vc.get("max_lora_rank", 16), "lora_request": LoRARequest.of(vc.get("lora_request"))}
    check_pool_size(out["max_loras"], out["max_lora_rank"])
    if out["lora_request"] is not None and not enable:
        raise ValueError("vllm_config lora_request needs enable_lora=True")
    return out


def check_pool_size(max_loras, max_lora_rank):
    if isinstance(max_loras, bool) or not isinstance(max_loras, int) or not 1 <= max_loras <= MAX_LORAS:
        raise ValueError(f"max_loras={max_loras!r} must be an integer in 1..{MAX_LORAS}")
    if isinstance(max_lora_rank, bool) or not isinstance(max_lora_rank, int) or not 1 <= max_lora_rank <= MAX_RANK:
        raise ValueError(f"max_lora_rank={max_lora_rank!r} must be an integer in 1..{MAX_RANK}")


# ---- the loader ----------------------------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Adapter:
    rank: int
    scale: float
    pairs: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]]      # (layer, module) -> (lora_A.weight [r, K], lora_B.weight [N, r]), bf16, on the host


_KEY = re.compile(r"^(?:base_model\.model\.)?(?:language_model\.)?model\.(?:language_model\.)?layers\.(\d+)\.(.+?)\.lora_([AB])(?:\.[A-Za-z0-9_\-]+)?\.weight$")


def module_shapes(config) -> Dict[str, Tuple[int, int]]:
    """{module: (N, K)} of the 7 Linears of a decoder layer of a Qwen2VLTextConfig."""
    D, I = config.hidden_size, config.intermediate_size
    QW, HW = config.num_attention_heads * 128, config.num_key_value_heads * 128
    return {"self_attn.q_proj": (QW, D), "self_attn.k_proj": (HW, D), "self_attn.v_proj": (HW, D), "self_attn.o_proj": (D, QW), "mlp.gate_proj": (I, D),
            "mlp.up_proj": (I, D), "mlp.down_proj": (D, I)}


def check_adapter_config(cfg: dict, max_lora_rank: int) -> Tuple[int, float]:
    """peft's adapter_config.json -> (r, scale).  Refused, each naming its field: use_dora, bias != "none", non-empty modules_to_save / rank_pattern /
    alpha_pattern, a peft_type other than LORA, r outside 1..max_lora_rank."""
    if not isinstance(cfg, dict) or "r" not in cfg:
        raise ValueError("LoRA adapter config: a dict with at least 'r' (peft's adapter_config.json)")
    if str(cfg.get("peft_type", "LORA")).upper() != "LORA":
        raise ValueError(f"LoRA adapter config: peft_type={cfg['peft_type']!r} is not served (LORA only)")
    if cfg.get("use_dora"):
        raise ValueError("LoRA adapter config: use_dora is not served by the HIP engine (the magnitude vector has no kernel)")
    if cfg.get("bias", "none") != "none":
        raise ValueError(f"LoRA adapter config: bias={cfg['bias']!r} is not served by the HIP engine (only 'none': adapters add no bias)")
    for field in ("modules_to_save", "rank_pattern", "alpha_pattern"):
        if cfg.get(field):
            raise ValueError(f"LoRA adapter config: a non-empty {field} ({cfg[field]!r}) is not served by the HIP engine (one rank and one alpha per adapter, no "
                             "retrained modules)")
    r = cfg["r"]
    if isinstance(r, bool) or not isinstance(r, int) or r < 1:
        raise ValueError(f"LoRA adapter config: r={r!r} must be an integer >= 1")
    if r > max_lora_rank:
        raise ValueError(f"LoRA adapter config: r={r} exceeds max_lora_rank={max_lora_rank} of this engine")
    alpha = float(cfg.get("lora_alpha", r))
    return r, alpha / (math.sqrt(r) if cfg.get("use_rslora") else r)


def parse_adapter(state_dict: Dict[str, torch.Tensor], cfg: dict, shapes: Dict[str, Tuple[int, int]], num_layers: int, max_lora_rank: int) -> Adapter:
    """A peft-layout state dict + config -> Adapter.  Refused, each naming the key: lora_embedding_* / embed_tokens / lm_head / visual.* keys, a key that is not
    a lora_A / lora_B weight of one of the 7 decoder Linears, a layer the model does not have, a lora_A without its lora_B (or the reverse), a shape that does
    not fit the module or the config's r.  Tensors of another float dtype are rounded to bf16 here, once."""
    r, scale = check_adapter_config(cfg, max_lora_rank)
    halves: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
    for key, t in state_dict.items():
        if "lora_embedding_" in key or "embed_tokens" in key or "lm_head" in key:
            raise ValueError(f"LoRA adapter: key '{key}' adapts the embeddings or lm_head, which the HIP engine never adapts")
        if re.search(r"(^|\.)visual\.", key):
            raise ValueError(f"LoRA adapter: key '{key}' adapts the vision tower (visual.*), which is not served: adapters cover the text decoder's Linears")
        m = _KEY.match(key)
        if m is None or m.group(2) not in shapes:
            raise ValueError(f"LoRA adapter: key '{key}' is not a lora_A / lora_B weight of a decoder Linear (model.layers.N.<{' | '.join(MODULES)}>.lora_A.weight)")
        layer, module, half = int(m.group(1)), m.group(2), m.group(3)
        if layer >= num_layers:
            raise ValueError(f"LoRA adapter: key '{key}' names layer {layer} of a model with {num_layers}")
        if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != 2:
            raise ValueError(f"LoRA adapter: key '{key}' must be a 2-D float tensor")
        N, K = shapes[module]
        want = (r, K) if half == "A" else (N, r)
        if tuple(t.shape) != want:
            raise ValueError(f"LoRA adapter: key '{key}' has shape {tuple(t.shape)}, but {module} with r={r} takes {want}")
        halves.setdefault((layer, module), {})[half] = (t.detach().to("cpu", torch.bfloat16).contiguous(), key)
    pairs = {}
    for (layer, module), h in sorted(halves.items()):
        if len(h) != 2:
            have = next(iter(h.values()))[1]
            raise ValueError(f"LoRA adapter: key '{have}' has no lora_{'B' if 'A' in h else 'A'} beside it")
        pairs[(layer, module)] = (h["A"][0], h["B"][0])
    if not pairs:
        raise ValueError("LoRA adapter: the state dict holds no lora_A / lora_B pair")
    return Adapter(r, scale, pairs)


def load_adapter_dir(path: str):
    """A peft directory -> (state dict, config dict): adapter_config.json + adapter_model.safetensors."""
    cfg_path, st_path = os.path.join(path, "adapter_config.json"), os.path.join(path, "adapter_model.safetensors")
    if not os.path.isfile(cfg_path) or not os.path.isfile(st_path):
        raise ValueError(f"LoRA adapter: '{path}' holds no adapter_config.json + adapter_model.safetensors")
    from safetensors.torch import load_file
    with open(cfg_path) as f:
        cfg = json.load(f)
    return load_file(st_path), cfg


# ---- the pool ------------------------------------------------------------------------------------------------------------------------------------------

class LoraPool:
    """Which adapter sits at which of the engine's max_loras places, and which cache slot runs under which adapter.

    known      lora_int_id -> (LoRARequest, Adapter): what add_lora registered (or a first use loaded from lora_path); the host copy stays, so a dropped
               adapter comes back with the bits it had
    resident   lora_int_id -> place, least recently used first
    slot_of    cache slot -> lora_int_id of the sequences that are live (a slot bound before its prefill until it is released)
    The three callbacks carry a decision out on the device: load(place, Adapter), remove(place), set_slot(slot, place or -1)."""

    def __init__(self, max_loras: int, max_lora_rank: int, load, remove, set_slot):
        check_pool_size(max_loras, max_lora_rank)
        self.max_loras, self.max_lora_rank = max_loras, max_lora_rank
        self._load, self._remove, self._set_slot = load, remove, set_slot
        self.known: Dict[int, Tuple[LoRARequest, Adapter]] = {}
        self.resident: "collections.OrderedDict[int, int]" = collections.OrderedDict()
        self.slot_of: Dict[int, int] = {}
        self.stats = {"loads": 0, "evictions": 0}

    def register(self, request: LoRARequest, adapter: Adapter):
        if request.lora_int_id in self.known:
            self.forget(request.lora_int_id)
        self.known[request.lora_int_id] = (request, adapter)

    def forget(self, lora_int_id: int) -> bool:
        """remove_lora: off the device and out of the registry.  A live sequence under it is an error."""
        if lora_int_id in self.slot_of.values():
            raise ValueError(f"remove_lora: adapter {lora_int_id} is used by a live sequence")
        place = self.resident.pop(lora_int_id, None)
        if place is not None:
            self._remove(place)
        return self.known.pop(lora_int_id, None) is not None

    def check_call(self, requests: List[Optional[LoRARequest]]):
        ids = sorted({r.lora_int_id for r in requests if r is not None})
        if len(ids) > self.max_loras:
            raise ValueError(f"the requests of one call name {len(ids)} distinct LoRA adapters (ids {ids}), max_loras={self.max_loras}: deferring requests "
                             "whose adapter does not fit is not built")

    def place(self, wanted: List[int]) -> Dict[int, int]:
        """Make every adapter of `wanted` resident -> {lora_int_id: place}.  A missing one takes a free place, or the place of the least recently used adapter
        that neither a live sequence nor this call uses."""
        wanted = list(dict.fromkeys(wanted))
        live = set(self.slot_of.values())
        if len(set(wanted) | live) > self.max_loras and any(w not in self.resident for w in wanted):
            raise ValueError(f"LoRA pool: adapters {sorted(set(wanted))} are wanted while live sequences use {sorted(live)}, max_loras={self.max_loras}: deferring "
                             "requests whose adapter does not fit is not built")
        for i in wanted:
            if i in self.resident:
                self.resident.move_to_end(i)
                continue
            used = set(self.resident.values())
            free = [p for p in range(self.max_loras) if p not in used]
            if free:
                place = free[0]
            else:
                victim = next(v for v in self.resident if v not in live and v not in wanted)      # (exists: checked above)
                place = self.resident.pop(victim)
                self._remove(place)
                self.stats["evictions"] += 1
            self._load(place, self.known[i][1])
            self.stats["loads"] += 1
            self.resident[i] = place
        return {i: self.resident[i] for i in wanted}

    def bind(self, slots: List[int], requests: List[Optional[LoRARequest]]):
        """Before a prefill: slot slots[j] runs request j's adapter (None: none)."""
        places = self.place([r.lora_int_id for r in requests if r is not None])
        for s, r in zip(slots, requests):
            s = int(s)
            if r is None:
                if self.slot_of.pop(s, None) is not None:
                    self._set_slot(s, -1)
            else:
                self.slot_of[s] = r.lora_int_id
                self._set_slot(s, places[r.lora_int_id])

    def inherit(self, src: int, dst_slots):
        """A fork / move: the destinations continue the source's sequence under its adapter (the device side does the same in td_qwen2_fork_slot)."""
        i = self.slot_of.get(int(src))
        for d in dst_slots:
            if i is None:
                self.slot_of.pop(int(d), None)
            else:
                self.slot_of[int(d)] = i

    def release(self, slots):
        """The sequences of these slots finished: the slots name no adapter."""
        for s in slots:
            if self.slot_of.pop(int(s), None) is not None:
                self._set_slot(int(s), -1)

    def release_all(self):
        self.release(list(self.slot_of))

    def clear_slots(self):
        """The slots were re-partitioned (the device map is cleared by td_qwen2_set_slots itself)."""
        self.slot_of.clear()
