"""FLUX IP-Adapter: image-prompt conditioning of the double-stream blocks on the HIP engine -- the specification and the checkpoint loader.

**Parity unpinned.**  `diffusers` is not installed here (tests/test_diffusers_probe.py); what follows is restated from the published diffusers
sources ([ext], >= 0.32): `attention_processor.FluxIPAdapterJointAttnProcessor2_0`, `transformer_flux.FluxTransformerBlock.forward`,
`embeddings.ImageProjection` / `MultiIPAdapterImageProjection`, `loaders.FluxIPAdapterMixin`, `loaders/transformer_flux.py`.  The CPU restatement the
tests run is tests/ip_adapter_common.py; the engine's arithmetic is spelled out in include/thinkdiff_hip.h (td_ip_attention_bf16, td_flux_ip_adapter_*).

Image projection, once per image, per adapter (J = joint_attention_dim, E = the image encoder's projection width):
    tokens = LayerNorm_J(Linear(embeds [n_img, E] -> [n_img, num_tokens * J]).reshape(n_img * num_tokens, J))       eps 1e-5, affine
    num_tokens = proj.weight.shape[0] / J        (published checkpoints: 4, 16 or 128)
Per double block i (single blocks get nothing), once per image:
    K_i = to_k_ip_i(tokens), V_i = to_v_ip_i(tokens)        Linear(J -> D, bias=True), split into heads of 128
Inside the block:
    ip_query = norm_q(to_q(norm_hidden))    the image stream's query before the concatenation with the text rows and BEFORE RoPE
    ip = 0;  for each adapter a in order:  ip += scale_a[i] * SDPA(ip_query, K_i^a, V_i^a)       no mask, scale 128^-0.5, every op a bf16 torch op;
                                                                                               `scale` is a Python float (an fp32 operand)
    hidden = hidden + gate_mlp * ff;  hidden = hidden + ip                                     ip is neither projected by to_out nor gated
The text stream is untouched.  `set_ip_adapter_scale` takes a float (all adapters, all blocks) or a list with one entry per adapter, each a float or
a list of `num_layers` per-block floats; a block whose scale is 0 contributes nothing.

Checkpoint forms `load_ip_adapter_state_dict` accepts (no hub access):
  * a local `.safetensors` file, or a directory plus `weight_name`;
  * the diffusers form  {"image_proj": {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}, "ip_adapter": {"{i}.to_k_ip.weight", ...}};
  * the XLabs file keys `ip_adapter_proj_model.{proj,norm}.{weight,bias}` and
    `double_blocks.{i}.processor.ip_adapter_double_stream_{k,v}_proj.{weight,bias}`.
The result is flat, under the engine's names: `image_proj.proj.weight`, ..., `ip_adapter.{i}.to_k_ip.weight`, ...

Not built: negative image prompts / true CFG with an image prompt, an image prompt together with reference tokens or a ControlNet, the
keywords in the other pipelines, a HIP image encoder (`ip_adapter_image` goes through a caller-supplied torch module).
"""
import os
import re
from typing import Dict, List, Optional, Sequence, Union

import torch

TD_IP_MAX_ADAPTERS = 4      # include/thinkdiff_hip.h
TD_IP_MAX_KEYS = 256

_XLABS_PROJ = re.compile(r"^ip_adapter_proj_model\.(proj|norm)\.(weight|bias)$")
_XLABS_BLOCK = re.compile(r"^double_blocks\.(\d+)\.processor\.ip_adapter_double_stream_(k|v)_proj\.(weight|bias)$")
_DIFF_BLOCK = re.compile(r"^(\d+)\.to_(k|v)_ip\.(weight|bias)$")
_PROJ_KEYS = ("proj.weight", "proj.bias", "norm.weight", "norm.bias")


def read_ip_adapter_file(path: str, weight_name: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The tensors of a local `.safetensors` file, or of `weight_name` inside a directory.  No hub."""
    from safetensors import safe_open
    if os.path.isdir(path):
        if not weight_name:
            raise ValueError(f"load_ip_adapter: {path!r} is a directory: weight_name= names the .safetensors file inside it")
        path = os.path.join(path, weight_name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path!r} is not a local IP-Adapter file (hub ids cannot be fetched here)")
    with safe_open(path, framework="pt") as fh:
        return {k: fh.get_tensor(k) for k in fh.keys()}


def xlabs_to_diffusers(sd: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
    """XLabs file keys -> the diffusers form; an unknown key is an error that names it."""
    out = {"image_proj": {}, "ip_adapter": {}}
    for k, v in sd.items():
        m = _XLABS_PROJ.match(k)
        if m:
            out["image_proj"][f"{m.group(1)}.{m.group(2)}"] = v
            continue
        m = _XLABS_BLOCK.match(k)
        if m:
            out["ip_adapter"][f"{int(m.group(1))}.to_{m.group(2)}_ip.{m.group(3)}"] = v
            continue
        raise KeyError(f"load_ip_adapter: unknown key {k!r} (expected ip_adapter_proj_model.* or double_blocks.<i>.processor.ip_adapter_double_stream_<k|v>_proj.*)")
    return out


def diffusers_to_xlabs(sd: Dict[str, Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    """The diffusers form -> XLabs file keys (the inverse of xlabs_to_diffusers)."""
    out = {}
    for k, v in sd["image_proj"].items():
        if k not in _PROJ_KEYS:
            raise KeyError(f"load_ip_adapter: unknown key 'image_proj.{k}'")
        out[f"ip_adapter_proj_model.{k}"] = v
    for k, v in sd["ip_adapter"].items():
        m = _DIFF_BLOCK.match(k)
        if not m:
            raise KeyError(f"load_ip_adapter: unknown key 'ip_adapter.{k}'")
        out[f"double_blocks.{int(m.group(1))}.processor.ip_adapter_double_stream_{m.group(2)}_proj.{m.group(3)}"] = v
    return out


def load_ip_adapter_state_dict(sd_or_path, weight_name: Optional[str] = None, *, num_layers: int, joint_dim: int, inner_dim: int):
    """-> (flat {engine name: tensor}, num_tokens, embed_dim), checked against the transformer: every key known, all `num_layers` double blocks
    present and no other, proj / norm over J = joint_dim, to_k_ip / to_v_ip [inner_dim, joint_dim].  Errors name the key."""
    sd = sd_or_path
    if not isinstance(sd, dict):
        sd = read_ip_adapter_file(str(sd), weight_name)
    if not ("image_proj" in sd and "ip_adapter" in sd and isinstance(sd["image_proj"], dict)):
        sd = xlabs_to_diffusers(sd)
    extra = [k for k in sd if k not in ("image_proj", "ip_adapter")]
    if extra:
        raise KeyError(f"load_ip_adapter: unknown key {extra[0]!r} beside 'image_proj' and 'ip_adapter'")
    flat: Dict[str, torch.Tensor] = {}
    for k, v in sd["image_proj"].items():
        if k not in _PROJ_KEYS:
            raise KeyError(f"load_ip_adapter: unknown key 'image_proj.{k}' (expected {', '.join(_PROJ_KEYS)})")
        flat["image_proj." + k] = v
    for k in _PROJ_KEYS:
        if "image_proj." + k not in flat:
            raise KeyError(f"load_ip_adapter: missing key 'image_proj.{k}'")
    blocks = set()
    for k, v in sd["ip_adapter"].items():
        m = _DIFF_BLOCK.match(k)
        if not m:
            raise KeyError(f"load_ip_adapter: unknown key 'ip_adapter.{k}' (expected <i>.to_k_ip.weight / .bias, <i>.to_v_ip.weight / .bias)")
        i = int(m.group(1))
        if i >= num_layers:
            raise ValueError(f"load_ip_adapter: 'ip_adapter.{k}' addresses double block {i}, the transformer has {num_layers}")
        blocks.add(i)
        flat[f"ip_adapter.{i}.to_{m.group(2)}_ip.{m.group(3)}"] = v
    for i in range(num_layers):
        for n in ("to_k_ip.weight", "to_k_ip.bias", "to_v_ip.weight", "to_v_ip.bias"):
            if f"ip_adapter.{i}.{n}" not in flat:
                raise ValueError(f"load_ip_adapter: missing key 'ip_adapter.{i}.{n}': the checkpoint covers {len(blocks)} double blocks, the transformer has {num_layers}")
    pw = flat["image_proj.proj.weight"]
    if pw.dim() != 2 or pw.shape[0] % joint_dim != 0 or pw.shape[0] == 0:
        raise ValueError(f"load_ip_adapter: 'image_proj.proj.weight' is {tuple(pw.shape)}: its rows must be num_tokens x J with J = joint_attention_dim = {joint_dim}")
    num_tokens, embed_dim = pw.shape[0] // joint_dim, pw.shape[1]
    want = {"image_proj.proj.bias": (num_tokens * joint_dim,), "image_proj.norm.weight": (joint_dim,), "image_proj.norm.bias": (joint_dim,)}
    for i in range(num_layers):
        for kv in ("k", "v"):
            want[f"ip_adapter.{i}.to_{kv}_ip.weight"] = (inner_dim, joint_dim)
            want[f"ip_adapter.{i}.to_{kv}_ip.bias"] = (inner_dim,)
    for k, shape in want.items():
        if tuple(flat[k].shape) != shape:
            raise ValueError(f"load_ip_adapter: {k!r} is {tuple(flat[k].shape)}, expected {shape} (J = {joint_dim}, D = {inner_dim})")
    return flat, num_tokens, embed_dim


def expand_scales(scale, n_adapters: int, num_layers: int) -> List[List[float]]:
    """diffusers' set_ip_adapter_scale argument -> per adapter the `num_layers` per-block floats: a float (all adapters, all blocks) or a list
    with one entry per adapter, each a float or a list of num_layers floats."""
    if isinstance(scale, (int, float)):
        scale = [float(scale)] * n_adapters
    scale = list(scale)
    if len(scale) != n_adapters:
        raise ValueError(f"set_ip_adapter_scale: {len(scale)} scales for {n_adapters} loaded adapters")
    out = []
    for a, s in enumerate(scale):
        if isinstance(s, (int, float)):
            out.append([float(s)] * num_layers)
            continue
        s = [float(v) for v in s]
        if len(s) != num_layers:
            raise ValueError(f"set_ip_adapter_scale: adapter {a}: {len(s)} per-block scales, the transformer has {num_layers} double blocks")
        out.append(s)
    return out


def normalize_image_embeds(embeds, n_adapters: int, batch: int, embed_dims: Sequence[int]) -> List[torch.Tensor]:
    """`ip_adapter_image_embeds` -> per adapter a tensor [batch', n_img, E] (batch' = 1 or the prompt batch): a tensor (one adapter) or a list with one
    entry per adapter, each [batch, n_img, E] or [n_img, E]."""
    if isinstance(embeds, torch.Tensor):
        embeds = [embeds]
    embeds = list(embeds)
    if len(embeds) != n_adapters:
        raise ValueError(f"ip_adapter_image_embeds: {len(embeds)} entries for {n_adapters} loaded adapters (one entry per adapter)")
    out = []
    for a, e in enumerate(embeds):
        if not isinstance(e, torch.Tensor) or e.dim() not in (2, 3):
            raise ValueError(f"ip_adapter_image_embeds[{a}] must be a tensor [batch, n_img, E] or [n_img, E]")
        if e.dim() == 2:
            e = e[None]
        if e.shape[-1] != embed_dims[a]:
            raise ValueError(f"ip_adapter_image_embeds[{a}] has width {e.shape[-1]}, adapter {a} projects embeddings of width {embed_dims[a]}")
        if e.shape[0] not in (1, batch):
            raise ValueError(f"ip_adapter_image_embeds[{a}] has batch {e.shape[0]}, the call has {batch} prompts")
        out.append(e)
    return out
