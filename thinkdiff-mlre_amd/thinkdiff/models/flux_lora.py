"""LoRA checkpoints for the FLUX transformer: state dict -> the engine's (parameter, lora_A, lora_B, scale) pairs.

**Parity unpinned**: restated from the published peft / diffusers source ([ext] peft `LoraLayer`, `LoraConfig`; [ext] diffusers
`FluxLoraLoaderMixin.lora_state_dict` / `load_lora_into_transformer`, `save_lora_weights`); neither package is on the build machine, so
nothing here was run against them.  This docstring is the specification the tests hold the parser to.

On this engine an adapter is always merged into the weights (`td_flux_lora_*` of include/thinkdiff_hip.h):
`W_eff = W + sum_i weight_i * (alpha_i / r_i) * lora_B_i @ lora_A_i`, recomputed from an untouched base copy whenever the adapters or their
weights change.  The parser only names, checks and scales; it moves no data to the device.

Accepted format -- what diffusers' `save_lora_weights` / peft's `get_peft_model_state_dict` write:

    [transformer.]<module>.lora_A.weight   [r, in_features]
    [transformer.]<module>.lora_B.weight   [out_features, r]
    [transformer.]<module>.alpha           scalar, optional

and the older diffusers spelling `<module>.lora.down.weight` (= lora_A) / `<module>.lora.up.weight` (= lora_B).  `<module>` is a Linear of
`FluxTransformer2DModel.param_table()` (`<module>.weight` is a 2-D parameter there): the attention projections, the MLPs, `proj_mlp` /
`proj_out` of the single blocks, the embedders, the adaLN Linears, the final `proj_out`.

`scale = alpha / r`, alpha taken from, in this order: the `alpha=` argument (a number, or a dict keyed by module name, with or without the
`transformer.` prefix -- a module missing from the dict falls through), a scalar `<module>.alpha` tensor, else `r` (scale 1, what diffusers
assumes for a file without alphas).  Safetensors metadata that describes a LoRA config (keys `lora_adapter_metadata`, `lora_alpha`, `r`,
`rank_pattern`, `alpha_pattern`, `peft_type`) is understood only in its simplest form -- a JSON object under `lora_adapter_metadata` (or the
flat keys) holding just `r` and `lora_alpha` as numbers and, optionally, empty `rank_pattern` / `alpha_pattern`, `use_dora: false`,
`target_modules`, `peft_type: "LORA"`, `bias: "none"`; then alpha = `lora_alpha` ranks below the two sources above it.  Anything else in such
metadata is refused unless `alpha=` is given: never a silently wrong scale.

Refused, with the offending key in the message (ValueError):
  * text-encoder keys (`text_encoder.*`, `text_encoder_2.*`): the text encoders take no adapters here;
  * `lora_B.bias`, any `.bias` or norm-scale delta, and every key that is none of the spellings above;
  * DoRA (`lora_magnitude_vector`);
  * kohya / BFL spellings (`lora_unet_*`, `double_blocks.*`, `single_blocks.*`, `*.lora_down.weight`, `*.lora_up.weight`): no key conversion;
  * a pair with only one half; a module that is not a Linear of the transformer;
  * shapes that do not fit the module, ranks that disagree between the halves;
  * a `lora_A` WIDER than the module's input -- the FLUX.1 Canny / Depth *LoRA* checkpoints, which widen `x_embedder` from 64 to 128 input
    channels: not built (load the full 128-channel Control checkpoints instead);
  * non-finite alpha.
"""
import json
import math
import os
from typing import Dict, Optional, Tuple, Union

import torch

_CONFIG_KEYS = ("lora_adapter_metadata", "lora_alpha", "r", "rank_pattern", "alpha_pattern", "peft_type")
_HARMLESS = {"target_modules": None, "peft_type": ("LORA",), "bias": ("none",), "use_dora": (False,), "rank_pattern": ({}, None),
             "alpha_pattern": ({}, None)}


def read_lora_file(path: str, weight_name: Optional[str] = None):
    """(state dict, metadata) of a local `.safetensors` file, or of `weight_name` (default `pytorch_lora_weights.safetensors`) inside a
    directory.  No hub."""
    from safetensors import safe_open
    if os.path.isdir(path):
        path = os.path.join(path, weight_name or "pytorch_lora_weights.safetensors")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path!r} is not a local LoRA file (hub ids cannot be fetched here)")
    with safe_open(path, framework="pt") as fh:
        return {k: fh.get_tensor(k) for k in fh.keys()}, (fh.metadata() or None)


def _metadata_alpha(metadata, have_alpha_arg: bool) -> Optional[float]:
    if not metadata or not any(k in metadata for k in _CONFIG_KEYS):
        return None
    if have_alpha_arg:
        return None      # the caller decides
    cfg = metadata
    if "lora_adapter_metadata" in metadata:
        try:
            cfg = json.loads(metadata["lora_adapter_metadata"])
        except (TypeError, ValueError):
            cfg = None
    if isinstance(cfg, dict) and "lora_alpha" in cfg and "r" in cfg:
        def val(v):
            if isinstance(v, str):
                try:
                    return json.loads(v)
                except ValueError:
                    return v
            return v
        rest = {k: val(v) for k, v in cfg.items() if k not in ("lora_alpha", "r", "format")}
        understood = all(k in _HARMLESS and (_HARMLESS[k] is None or v in _HARMLESS[k]) for k, v in rest.items())
        a = val(cfg["lora_alpha"])
        if understood and isinstance(a, (int, float)) and not isinstance(a, bool):
            return float(a)
    raise ValueError(f"LoRA metadata describes an adapter config this parser does not fully understand (keys {sorted(metadata)}): "
                     "pass alpha= (a number, or a dict per module) to fix the scale explicitly")


def parse_lora_state_dict(sd: Dict[str, torch.Tensor], metadata: Optional[dict] = None, alpha: Union[None, float, Dict[str, float]] = None,
                          linear_shapes: Optional[Dict[str, Tuple[int, int]]] = None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor, float]]:
    """{engine parameter name `<module>.weight`: (lora_A [r, in], lora_B [out, r], alpha / r)}; see the module docstring.
    linear_shapes: {`<module>.weight`: (out_features, in_features)} of the target transformer (FluxTransformer2DModel.linear_shapes());
    None skips the module / shape checks that need it (key spelling, halves and ranks are checked regardless)."""
    meta_alpha = _metadata_alpha(metadata, alpha is not None)
    halves: Dict[str, Dict[str, torch.Tensor]] = {}
    alphas: Dict[str, torch.Tensor] = {}
    for key, t in sd.items():
        if key.startswith(("text_encoder.", "text_encoder_2.")):
            raise ValueError(f"LoRA key {key!r}: text-encoder adapters are not built (transformer keys only)")
        if "lora_magnitude_vector" in key:
            raise ValueError(f"LoRA key {key!r}: DoRA (lora_magnitude_vector) is not built")
        if key.startswith("lora_unet_") or key.startswith(("double_blocks.", "single_blocks.")) or ".double_blocks." in key or ".single_blocks." in key \
                or key.endswith((".lora_down.weight", ".lora_up.weight")):
            raise ValueError(f"LoRA key {key!r}: kohya / BFL key spellings are not converted (save the adapter in diffusers / peft format)")
        k = key[len("transformer."):] if key.startswith("transformer.") else key
        for suffix, half in ((".lora_A.weight", "A"), (".lora_B.weight", "B"), (".lora.down.weight", "A"), (".lora.up.weight", "B")):
            if k.endswith(suffix):
                mod = k[:-len(suffix)]
                if half in halves.setdefault(mod, {}):
                    raise ValueError(f"LoRA key {key!r}: a second lora_{half} for module {mod!r}")
                halves[mod][half] = t
                break
        else:
            if k.endswith(".alpha"):
                alphas[k[:-len(".alpha")]] = t
            elif k.endswith((".bias", ".weight", ".scale")):      # lora_B.bias, diff_b, a norm's weight / scale delta
                raise ValueError(f"LoRA key {key!r}: bias and norm-scale deltas are not built (low-rank pairs on Linear weights only)")
            else:
                raise ValueError(f"LoRA key {key!r}: not a lora_A / lora_B / alpha key of the diffusers / peft format")
    out = {}
    for mod, h in halves.items():
        if "A" not in h or "B" not in h:
            raise ValueError(f"LoRA module {mod!r}: only lora_{'A' if 'A' in h else 'B'} is present (a pair needs both halves)")
        A, B = h["A"], h["B"]
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[1] or A.shape[0] < 1:
            raise ValueError(f"LoRA module {mod!r}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} are not [r, in] / [out, r] with one rank r >= 1")
        r = A.shape[0]
        name = mod + ".weight"
        if linear_shapes is not None:
            if name not in linear_shapes:
                raise ValueError(f"LoRA module {mod!r}: not a Linear of this transformer")
            out_f, in_f = linear_shapes[name]
            if A.shape[1] > in_f:
                raise ValueError(f"LoRA module {mod!r}: lora_A reads {A.shape[1]} input channels, the module has {in_f} -- adapters that widen a Linear "
                                 "(the FLUX.1 Canny / Depth LoRA checkpoints on x_embedder) are not built; load the full Control checkpoint")
            if A.shape[1] != in_f or B.shape[0] != out_f:
                raise ValueError(f"LoRA module {mod!r}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not fit the module's weight [{out_f}, {in_f}]")
        a = None
        if isinstance(alpha, dict):
            a = alpha.get(mod, alpha.get("transformer." + mod))
        elif alpha is not None:
            a = alpha
        if a is None and mod in alphas:
            t = alphas[mod]
            if t.numel() != 1:
                raise ValueError(f"LoRA key {mod + '.alpha'!r}: alpha must be a scalar, got shape {tuple(t.shape)}")
            a = float(t.float().item())
        if a is None:
            a = meta_alpha if meta_alpha is not None else float(r)
        a = float(a)
        if not math.isfinite(a):
            raise ValueError(f"LoRA module {mod!r}: alpha = {a} is not finite")
        out[name] = (A, B, a / r)
    for mod in alphas:
        if mod not in halves:
            raise ValueError(f"LoRA key {mod + '.alpha'!r}: an alpha without its lora_A / lora_B pair")
    if not out:
        raise ValueError("LoRA state dict holds no lora_A / lora_B pair")
    return out
