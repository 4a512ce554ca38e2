"""FLUX.1 MMDiT on the HIP engine (libthinkdiff_hip.so `td_flux_*`).

Host-side mirror of the object the reference drivers reach through `diffusion_pipe.transformer`
([ext] diffusers 0.31.0 `FluxTransformer2DModel`): same config keys, same state-dict names, same
`forward(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids,
guidance)` meaning.  All compute happens in the C++/HIP engine; this class only owns the handle,
moves checkpoints into the engine's fused weight arena and converts arguments to device pointers.
"""
import ctypes
import dataclasses
import glob
import json
import os
from typing import Dict, Optional, Sequence

import torch

from .. import _hip
from ..ops import register as _register_ops

_OPS = _register_ops()      # torch.ops.thinkdiff_hip: the denoise loop is dispatched as custom ops over the C ABI (GPU kernels only, no fallback)


@dataclasses.dataclass
class FluxTransformerConfig:
    """Keys of [ext] FLUX.1-dev transformer/config.json."""
    patch_size: int = 1
    in_channels: int = 64
    num_layers: int = 19
    num_single_layers: int = 38
    attention_head_dim: int = 128
    num_attention_heads: int = 24
    joint_attention_dim: int = 4096
    pooled_projection_dim: int = 768
    guidance_embeds: bool = True
    axes_dims_rope: Sequence[int] = (16, 56, 56)
    # [ext] diffusers >= 0.32: null / absent = in_channels.  FLUX.1 Fill (in 384, out 64) and FLUX.1 Canny / Depth (in 128, out 64) read a
    # per-image condition of in_channels - out_channels columns concatenated to the latents (FluxTransformer2DModel.set_channel_condition).
    out_channels: Optional[int] = None

    @property
    def inner_dim(self):
        return self.attention_head_dim * self.num_attention_heads

    @property
    def latent_channels(self) -> int:
        """Width of the packed latents and of the velocity (proj_out's)."""
        return self.out_channels or self.in_channels

    @property
    def cond_channels(self) -> int:
        """Width of the channel condition x_embedder reads beside the latents (0: an unconditioned model)."""
        return self.in_channels - self.latent_channels

    def to_hip(self) -> "_hip.TdFluxConfig":
        """The engine's `struct TdFluxConfig` (out_channels None -> 0, the struct's spelling of "= in_channels")."""
        return _hip.TdFluxConfig(self.in_channels, self.num_layers, self.num_single_layers, self.num_attention_heads,
                                 self.attention_head_dim, self.joint_attention_dim, self.pooled_projection_dim,
                                 int(self.guidance_embeds), 4, (ctypes.c_int * 3)(*self.axes_dims_rope), 10000.0, int(self.out_channels or 0))


@dataclasses.dataclass
class FirstBlockCacheConfig:
    """[ext] diffusers >= 0.33 `FirstBlockCacheConfig`: a denoise step whose first transformer block moved its output by no more than
    `threshold` (relative mean absolute change of the block's residual against the last computed step's) reuses what the remaining blocks
    added at that step instead of running them.  0 = always compute; diffusers suggests 0.05 - 0.2 for FLUX."""
    threshold: float = 0.05

    def __post_init__(self):
        t = self.threshold
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not t >= 0:      # (NaN fails the comparison)
            raise ValueError(f"FirstBlockCacheConfig: threshold = {t!r} must be a number >= 0")
        self.threshold = float(t)


def apply_first_block_cache(transformer: "FluxTransformer2DModel", config: Optional[FirstBlockCacheConfig] = None) -> "FluxTransformer2DModel":
    """[ext] diffusers `apply_first_block_cache(module, config)`: the same as `transformer.enable_cache(config)`."""
    transformer.enable_cache(config or FirstBlockCacheConfig())
    return transformer


def effective_scalar(value: float, dtype: torch.dtype) -> float:
    """What the sinusoidal embedding finally sees for `timestep`/`guidance` in the reference pipeline:
    cast to the latents dtype, /1000 in the pipeline, *1000 in the transformer, all in `dtype`
    ([ext] pipeline_flux.py `timestep / 1000`, transformer_flux.py `timestep.to(dtype) * 1000`)."""
    x = torch.tensor([value], dtype=torch.float32).to(dtype)
    return float(((x / 1000).to(dtype) * 1000).float())


class FluxTransformer2DModel:
    dtype = torch.bfloat16

    def __init__(self, config: Optional[FluxTransformerConfig] = None, max_img_tokens: int = 4096,
                 max_txt_tokens: int = 512, max_steps: int = 64, device="cuda", **config_kwargs):
        self.config = config or FluxTransformerConfig(**config_kwargs)
        c = self.config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _hip.ThinkDiffHipError("FluxTransformer2DModel runs on the MI355X HIP engine only (device='cuda')")
        self._L = _hip.lib()
        cc = c.to_hip()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _hip.check(self._L.td_flux_create(ctypes.byref(cc), max_img_tokens, max_txt_tokens, max_steps, ctypes.byref(h)))
        self._h = h
        self.max_img_tokens, self.max_txt_tokens, self.max_steps = max_img_tokens, max_txt_tokens, max_steps
        self._n_steps = 0

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.td_flux_destroy(h)

    def fork(self) -> "FluxTransformer2DModel":
        """A second context over the same weights (own workspace / conditioning / schedule) for images in flight on
        another stream.  Keeps a reference to the parent, which owns the weights and the precision setting."""
        child = object.__new__(type(self))
        child.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _hip.check(self._L.td_flux_fork(self._h, ctypes.byref(h)))
        child._h, child._parent, child._n_steps = h, self, 0
        return child

    @staticmethod
    def denoise_multi(contexts, latents, sigmas: Sequence[float], streams, inpaint=None):
        """td_flux_denoise for several prepared contexts at once, context k on streams[k] (torch.cuda.Stream).  inpaint: None, or one
        (image_latents, noise, mask) triple per context -- the inpainting step of `denoise` for each."""
        engines, sg, ss = [int(m._h.value) for m in contexts], [float(s) for s in sigmas], [int(st.cuda_stream) for st in streams]
        if inpaint is None:
            _OPS.flux_denoise_multi_(engines, list(latents), sg, ss)
        else:
            z, noise, mask = (list(t) for t in zip(*inpaint))
            _OPS.flux_denoise_multi_inpaint_(engines, list(latents), sg, z, noise, mask, ss)
        return latents

    # ---- parameters ---------------------------------------------------------------------------------
    def param_table(self) -> Dict[str, int]:
        n = self._L.td_flux_num_params(self._h)
        buf = ctypes.create_string_buffer(256)
        cnt = ctypes.c_int64()
        out = {}
        for i in range(n):
            _hip.check(self._L.td_flux_param_info(self._h, i, buf, 256, ctypes.byref(cnt)))
            out[buf.value.decode()] = cnt.value
        return out

    def num_parameters(self) -> int:
        return sum(self.param_table().values())

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        table = self.param_table()
        missing = [k for k in table if k not in sd]
        unexpected = [k for k in sd if k not in table]
        if strict and (missing or unexpected):
            raise KeyError(f"FluxTransformer2DModel.load_state_dict: missing={missing[:4]}.. unexpected={unexpected[:4]}..")
        for name, t in sd.items():
            if name not in table:
                continue
            d = t.to(device=self.device, dtype=torch.bfloat16).contiguous()
            _hip.check(self._L.td_flux_load_param(self._h, name.encode(), _hip.ptr(d), d.numel(), _hip.stream_ptr()))
            torch.cuda.current_stream().synchronize()  # `d` may be a temporary
        return missing, unexpected

    @staticmethod
    def config_from_json(raw: dict) -> FluxTransformerConfig:
        """transformer/config.json -> FluxTransformerConfig: known keys only; `out_channels` absent or null = in_channels."""
        fields = {f.name for f in dataclasses.fields(FluxTransformerConfig)}
        return FluxTransformerConfig(**{k: v for k, v in raw.items() if k in fields})

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str = "transformer", **kw):
        """Local directories only (there is no hub access): <path>/<subfolder>/{config.json,*.safetensors}."""
        from safetensors import safe_open
        root = os.path.join(path, subfolder) if os.path.isdir(os.path.join(path, subfolder)) else path
        with open(os.path.join(root, "config.json")) as fh:
            raw = json.load(fh)
        model = cls(cls.config_from_json(raw), **kw)
        seen = set()
        for fn in sorted(glob.glob(os.path.join(root, "*.safetensors"))):
            with safe_open(fn, framework="pt") as fh:
                part = {k: fh.get_tensor(k) for k in fh.keys()}
            model.load_state_dict(part, strict=False)
            seen.update(part)
        missing = [k for k in model.param_table() if k not in seen]
        if missing:
            raise KeyError(f"checkpoint at {root} lacks {len(missing)} tensors, e.g. {missing[:3]}")
        return model

    # ---- LoRA adapters (td_flux_lora_*: always merged, recomputed from a base copy) ----------------------
    def linear_shapes(self) -> Dict[str, tuple]:
        """{`<module>.weight`: (out_features, in_features)} of every Linear (the parameters an adapter may target)."""
        out = {}
        rows, cols = ctypes.c_int64(), ctypes.c_int64()
        for name in self.param_table():
            _hip.check(self._L.td_flux_param_shape(self._h, name.encode(), ctypes.byref(rows), ctypes.byref(cols)))
            if name.endswith(".weight") and cols.value > 1:
                out[name] = (rows.value, cols.value)
        return out

    def read_param(self, name: str) -> torch.Tensor:
        """The parameter as the forward sees it now (base + merged adapters): a new device tensor, [N, K] for a Linear's weight."""
        with torch.cuda.device(self.device):
            return _OPS.flux_read_param(int(self._root()._h.value), name)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Effective weights under the diffusers names (what `transformer.state_dict()` is after diffusers' fuse_lora)."""
        return {name: self.read_param(name) for name in self.param_table()}

    def _root(self) -> "FluxTransformer2DModel":
        return getattr(self, "_parent", None) or self

    def _lora_state(self) -> dict:
        r = self._root()
        if not hasattr(r, "_lora_active"):
            r._lora_loaded, r._lora_active = [], {}      # names in load order; {name: weight} of the active set
        return r.__dict__

    def _apply_adapters(self):
        st = self._lora_state()
        names = [n for n in st["_lora_loaded"] if n in st["_lora_active"]]
        with torch.cuda.device(self.device):
            _OPS.flux_lora_set_adapters(int(self._root()._h.value), names, [float(st["_lora_active"][n]) for n in names])
        # (in an 8-bit mode the engine has quantised the merged weights again under the precision settings it holds)

    def load_lora_adapter(self, sd_or_path, adapter_name: str = "default", alpha=None, weight_name: Optional[str] = None):
        """diffusers' `transformer.load_lora_adapter`: parse (thinkdiff.models.flux_lora), copy every pair into the engine, then activate the
        adapter at weight 1.0 together with those already active.  sd_or_path: a state dict, a local .safetensors file, or a directory
        (+ weight_name)."""
        from . import flux_lora
        if getattr(self, "_parent", None) is not None:
            raise _hip.ThinkDiffHipError("load_lora_adapter: adapters belong to the parent transformer (forks share its weights)")
        st = self._lora_state()
        if adapter_name in st["_lora_loaded"]:
            raise ValueError(f"adapter {adapter_name!r} is already loaded (delete_adapters first, or pick another adapter_name)")
        metadata = None
        if not isinstance(sd_or_path, dict):
            sd_or_path, metadata = flux_lora.read_lora_file(str(sd_or_path), weight_name)
        pairs = flux_lora.parse_lora_state_dict(sd_or_path, metadata, alpha, self.linear_shapes())
        h = int(self._h.value)
        try:
            with torch.cuda.device(self.device):
                for name, (A, B, scale) in pairs.items():
                    a = A.to(self.device, torch.bfloat16).contiguous()
                    b = B.to(self.device, torch.bfloat16).contiguous()
                    _OPS.flux_lora_load(h, adapter_name, name, a, b, float(scale))
                torch.cuda.current_stream().synchronize()      # `a` / `b` may be temporaries
        except Exception:
            try:
                _OPS.flux_lora_delete(h, adapter_name)      # no half-loaded adapter stays behind
            except RuntimeError:
                pass
            raise
        st["_lora_loaded"].append(adapter_name)
        st["_lora_active"][adapter_name] = 1.0
        self._apply_adapters()
        return sorted(pairs)

    def set_adapters(self, names, weights=None):
        """diffusers' set_adapters: the active set and its weights (default 1.0 each); every touched parameter is recomputed from its base."""
        st = self._lora_state()
        names = [names] if isinstance(names, str) else list(names)
        if weights is None:
            weights = [1.0] * len(names)
        elif isinstance(weights, (int, float)):
            weights = [float(weights)] * len(names)
        weights = list(weights)
        if len(weights) != len(names):
            raise ValueError(f"set_adapters: {len(names)} adapter names, {len(weights)} weights")
        for n in names:
            if n not in st["_lora_loaded"]:
                raise ValueError(f"set_adapters: unknown adapter {n!r} (loaded: {st['_lora_loaded']})")
        for w in weights:
            if not isinstance(w, (int, float)):
                raise ValueError("set_adapters: per-block weight dicts are not built; one number per adapter")
        st["_lora_active"] = {n: float(w) for n, w in zip(names, weights)}
        self._apply_adapters()

    def delete_adapters(self, names):
        st = self._lora_state()
        names = [names] if isinstance(names, str) else list(names)
        for n in names:
            if n not in st["_lora_loaded"]:
                raise ValueError(f"delete_adapters: unknown adapter {n!r} (loaded: {st['_lora_loaded']})")
        with torch.cuda.device(self.device):
            for n in names:
                _OPS.flux_lora_delete(int(self._root()._h.value), n)
                st["_lora_loaded"].remove(n)
                st["_lora_active"].pop(n, None)

    def unload_lora(self):
        """diffusers' unload_lora_weights: drop every adapter; each parameter gets its base bits back."""
        st = self._lora_state()
        with torch.cuda.device(self.device):
            _OPS.flux_lora_delete(int(self._root()._h.value), "")
        st["_lora_loaded"], st["_lora_active"] = [], {}

    def active_adapters(self) -> Dict[str, float]:
        st = self._lora_state()
        return {n: st["_lora_active"][n] for n in st["_lora_loaded"] if n in st["_lora_active"]}

    def list_adapters(self):
        return list(self._lora_state()["_lora_loaded"])

    def lora_info(self) -> Dict[str, int]:
        n, p, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _hip.check(self._L.td_flux_lora_info(self._h, ctypes.byref(n), ctypes.byref(p), ctypes.byref(b)))
        return {"adapters": n.value, "params_touched": p.value, "bytes_held": b.value}

    def init_random(self, seed: int = 0, std: float = 0.02):
        """Synthetic full-shape checkpoint generated on the device (throughput runs)."""
        _hip.check(self._L.td_flux_init_random(self._h, seed, std, _hip.stream_ptr()))
        return self

    FP8_GEMMS = {"qkv": 1, "out": 2, "ff1": 4, "ff2": 8, "single_in": 16, "single_out": 32}     # TD_FP8_* of include/thinkdiff_hip.h

    def set_attention(self, mode: str = "bf16"):
        """Arithmetic of the joint attention: "bf16" (default, the reference graph's) or "fp8" (QK^T and P.V on the e4m3 matrix
        instruction, td_flux_set_attention(TD_ATTENTION_FP8)); independent of set_precision, meant for the 8-bit modes."""
        _hip.check(self._L.td_flux_set_attention(self._h, {"bf16": 0, "fp8": 1}[mode]))
        self.attention = mode
        return self

    def set_precision(self, precision: str = "bf16", fp8_gemms=None, act_scales: str = "dynamic", smoothing: bool = False):
        """"bf16" (default) or "fp8": e4m3 operands for the block GEMMs (weights quantised per output channel from the
        parameters as loaded now -- call after load_state_dict / init_random; activations per token on the fly).
        fp8_gemms: None = every block Linear, or the classes that take the fp8 path (names of FP8_GEMMS, or the bit mask);
        the others stay bf16."""
        code = {"bf16": 0, "bfloat16": 0, "fp8": 1, "fp8_e4m3": 1, "float8_e4m3fn": 1, "int8": 2, "w8a8": 2}[str(precision).replace("torch.", "")]
        _hip.check(self._L.td_flux_set_precision(self._h, code, _hip.stream_ptr()))
        mask = 63 if fp8_gemms is None else (int(fp8_gemms) if isinstance(fp8_gemms, int) else sum(self.FP8_GEMMS[str(n)] for n in fp8_gemms))
        _hip.check(self._L.td_flux_set_fp8_gemms(self._h, mask))
        # int8 only: "history" = per-token scales of the MLP operands from the previous denoise step (td_flux_set_act_scales)
        _hip.check(self._L.td_flux_set_act_scales(self._h, {"dynamic": 0, "history": 1}[act_scales] if code == 2 else 0))
        # int8 only: per-channel smoothing of outlier-carrying activations, calibrated on the first forward (td_flux_set_smoothing)
        _hip.check(self._L.td_flux_set_smoothing(self._h, 1 if (smoothing and code == 2) else 0))
        self.precision, self.fp8_gemms, self.act_scales = ("bf16", "fp8", "int8")[code], mask, (act_scales if code == 2 else "dynamic")
        self.smoothing = bool(smoothing and code == 2)
        return self

    # ---- conditioning / schedule ----------------------------------------------------------------------
    def set_condition(self, prompt_embeds, pooled, img_ids, txt_ids=None):
        assert prompt_embeds.dim() == 2 and pooled.dim() == 1, "one prompt per call: [T,joint], [pooled]"
        pe = prompt_embeds.to(self.device, torch.bfloat16).contiguous()
        po = pooled.to(self.device, torch.bfloat16).contiguous()
        ii = img_ids.to(self.device, torch.float32).contiguous()
        ti = None if txt_ids is None else txt_ids.to(self.device, torch.float32).contiguous()
        _hip.check(self._L.td_flux_set_condition(self._h, _hip.ptr(pe), pe.shape[0], _hip.ptr(po), _hip.ptr(ti),
                                                 _hip.ptr(ii), ii.shape[0], _hip.stream_ptr()))
        self._n_img = ii.shape[0]
        torch.cuda.current_stream().synchronize()

    def set_channel_condition(self, cond):
        """The per-image condition of a channel-conditioned model, cond [S_img, in_channels - out_channels] bf16 (FLUX.1 Fill: packed
        masked-image latents | unshuffled mask; FLUX.1 Canny / Depth: the packed control-image latents): what diffusers concatenates to
        the latents in front of every transformer call.  After set_condition, once per image; this context's own (forks hold theirs)."""
        c = self.config
        if c.cond_channels == 0:
            raise _hip.ThinkDiffHipError(f"this transformer takes no channel condition (in_channels = out_channels = {c.in_channels})")
        assert cond.dim() == 2 and cond.shape[1] == c.cond_channels, f"cond must be [S_img, {c.cond_channels}], got {tuple(cond.shape)}"
        d = cond.to(self.device, torch.bfloat16).contiguous()
        _OPS.flux_set_channel_condition(int(self._h.value), d)
        torch.cuda.current_stream().synchronize()      # `d` may be a temporary

    def set_reference_tokens(self, ref_latents, ref_ids=None):
        """FLUX.1 Kontext's reference tokens of one image: ref_latents [S_ref, out_channels] bf16 (packed, shifted / scaled image latents),
        ref_ids [S_ref, 3] (first coordinate 1).  From now on every forward of this context runs over [text | latents | reference] and
        returns the velocity of the latents' rows only -- what diffusers' FluxKontextPipeline does with a torch.cat and a slice per step.
        After set_condition (which always voids them), once per image; this context's own (forks hold theirs).  None clears."""
        c = self.config
        if ref_latents is None:
            ref_latents = torch.empty(0, c.latent_channels, dtype=torch.bfloat16, device=self.device)
            ref_ids = torch.empty(0, 3, dtype=torch.float32, device=self.device)
        if ref_ids is None:
            raise ValueError("set_reference_tokens: ref_ids [S_ref, 3] are required with ref_latents (only set_reference_tokens(None) clears)")
        assert ref_latents.dim() == 2 and ref_latents.shape[1] == c.latent_channels, f"ref_latents must be [S_ref, {c.latent_channels}], got {tuple(ref_latents.shape)}"
        d = ref_latents.to(self.device, torch.bfloat16).contiguous()
        ii = ref_ids.to(self.device, torch.float32).contiguous()
        _OPS.flux_set_reference_tokens(int(self._h.value), d, ii)
        torch.cuda.current_stream().synchronize()      # `d` / `ii` may be temporaries

    def set_timesteps(self, t_eff: Sequence[float], g_eff: float = 0.0):
        arr = (ctypes.c_float * len(t_eff))(*[float(t) for t in t_eff])
        _hip.check(self._L.td_flux_set_timesteps(self._h, ctypes.cast(arr, ctypes.c_void_p), len(t_eff), float(g_eff), _hip.stream_ptr()))
        self._n_steps = len(t_eff)

    def forward_step(self, latents, step: int, out=None):
        assert latents.dtype == torch.bfloat16 and latents.is_contiguous() and latents.shape == (self._n_img, self.config.latent_channels)
        if out is None:
            out = torch.empty_like(latents)
        return _OPS.flux_forward_(int(self._h.value), latents, int(step), out)

    def denoise(self, latents, sigmas: Sequence[float], inpaint=None):
        """In-place Euler flow-matching loop over the prepared timesteps (len(sigmas) == n_steps + 1).  inpaint: an (image_latents,
        noise, mask) triple of [S_img, out_channels] bf16 tensors -- FluxInpaintPipeline's loop: after every step the latents are blended
        with the image latents re-noised to the next sigma under the mask (flux_inpaint_step_)."""
        assert latents.dtype == torch.bfloat16 and latents.is_contiguous() and latents.shape == (self._n_img, self.config.latent_channels)
        if inpaint is None:
            return _OPS.flux_denoise_(int(self._h.value), latents, [float(s) for s in sigmas])
        z, noise, mask = inpaint
        return _OPS.flux_denoise_inpaint_(int(self._h.value), latents, [float(s) for s in sigmas], z, noise, mask)

    def denoise_cfg(self, neg_context, latents, sigmas: Sequence[float], scale: float):
        """FluxKontextPipeline's loop under true classifier-free guidance, in place: per step the transformer on this (positive) context
        and on `neg_context` (a fork prepared with the negative prompt and the same schedule), then flux_cfg_step_ --
        v = v_neg + scale * (v_pos - v_neg) and the Euler step, fused.  One stream."""
        assert latents.dtype == torch.bfloat16 and latents.is_contiguous() and latents.shape == (self._n_img, self.config.latent_channels)
        return _OPS.flux_denoise_cfg_(int(self._h.value), int(neg_context._h.value), latents, [float(s) for s in sigmas], float(scale))

    # ---- first-block cache (td_flux_set_block_cache*; the names of diffusers' CacheMixin) ---------------------------
    def _cache_root(self, what: str) -> "FluxTransformer2DModel":
        if getattr(self, "_parent", None) is not None:
            raise _hip.ThinkDiffHipError(f"{what}: the cache settings belong to the parent transformer (forks follow it)")
        return self

    def enable_cache(self, config: Optional[FirstBlockCacheConfig] = None):
        """Skip the blocks behind the first on denoise steps where its residual changed by no more than `config.threshold` (FirstBlockCacheConfig).
        The setting is the model's: every pipeline built on this transformer honours it, forks included; each context (image in flight, CFG
        branch) keeps its own state, reset at the start of every denoise loop.  Costs one host synchronisation per forward while enabled."""
        config = config or FirstBlockCacheConfig()
        if not isinstance(config, FirstBlockCacheConfig):
            raise ValueError(f"enable_cache: config is a {type(config).__name__}; only FirstBlockCacheConfig is built (no TeaCache, FasterCache or "
                             "PyramidAttentionBroadcast)")
        r = self._cache_root("enable_cache")
        _hip.check(self._L.td_flux_set_block_cache(r._h, 1, float(config.threshold)))
        r._cache_config, r._cache_schedule = config, None
        return self

    def set_cache_schedule(self, compute: Sequence):
        """A fixed schedule instead of the threshold: forward i of every denoise loop (counted from the state's last reset) runs all blocks where
        compute[i] is true and reuses the last computed forward's tail where it is false; forwards beyond the list are computed.  compute[0]
        must be true.  The metric is still taken and logged (cache_stats)."""
        r = self._cache_root("set_cache_schedule")
        flags = bytes(1 if c else 0 for c in compute)
        _hip.check(self._L.td_flux_set_block_cache_schedule(r._h, flags, len(flags)))
        r._cache_config, r._cache_schedule = None, [bool(c) for c in compute]
        return self

    def disable_cache(self):
        r = self._cache_root("disable_cache")
        _hip.check(self._L.td_flux_set_block_cache(r._h, 0, 0.0))
        r._cache_config = r._cache_schedule = None
        return self

    @property
    def is_cache_enabled(self) -> bool:
        r = self._root()
        return getattr(r, "_cache_config", None) is not None or getattr(r, "_cache_schedule", None) is not None

    def reset_cache(self):
        """Forget THIS context's cache state and log (every denoise loop does so at its start)."""
        _hip.check(self._L.td_flux_block_cache_reset(self._h))

    def cache_stats(self):
        """(metrics, computed) of THIS context's forwards since its state was last reset: the first-block metric of each (inf where there was no
        previous residual) and whether all blocks ran."""
        n = ctypes.c_int()
        _hip.check(self._L.td_flux_block_cache_stats(self._h, 0, None, None, ctypes.byref(n)))
        cap = max(1, n.value)
        met, comp = (ctypes.c_float * cap)(), (ctypes.c_ubyte * cap)()
        _hip.check(self._L.td_flux_block_cache_stats(self._h, cap, ctypes.cast(met, ctypes.c_void_p), ctypes.cast(comp, ctypes.c_void_p), ctypes.byref(n)))
        k = min(cap, n.value)
        return [float(met[i]) for i in range(k)], [bool(comp[i]) for i in range(k)]

    # ---- ControlNet (thinkdiff.models.flux_controlnet) ------------------------------------------------------
    def attach_controlnet(self, controlnet):
        """Attach one `FluxControlNetModel` context to THIS context (None detaches): every forward / denoise step whose scale is not 0
        then runs the ControlNet first and adds its scaled samples behind the blocks (td_flux_attach_controlnet).  One ControlNet context
        serves one transformer context at a time (fork both: one pair per image in flight).  The scales return to 1.0."""
        _hip.check(self._L.td_flux_attach_controlnet(self._h, controlnet._h if controlnet is not None else None))
        self._controlnet = controlnet      # (keeps the attached context alive)
        return self

    def attach_controlnets(self, controlnets):
        """Attach 0 .. 4 `FluxControlNetModel` contexts to THIS context, in list order (empty: detach all): at every step the nets whose
        scale is not 0 run one after another and the bf16 left fold of their scaled samples is added behind each block, one launch
        (td_flux_attach_controlnets).  The same context may not appear twice -- list forks of it.  Every scale table returns to 1.0."""
        cns = list(controlnets)
        arr = (ctypes.c_void_p * max(1, len(cns)))(*[c._h.value for c in cns])
        _hip.check(self._L.td_flux_attach_controlnets(self._h, ctypes.cast(arr, ctypes.c_void_p), len(cns)))
        self._controlnet = cns or None      # (keeps the attached contexts alive)
        return self

    def attached_controlnets(self) -> int:
        n = ctypes.c_int()
        _hip.check(self._L.td_flux_attached_controlnets(self._h, ctypes.byref(n)))
        return n.value

    def set_controlnet_scales(self, scales: Sequence[float], net: Optional[int] = None):
        """The conditioning scale of every prepared step: `controlnet_conditioning_scale * controlnet_keep[i]` (0: the plain step);
        `net`: which of the attached ControlNets (td_flux_set_controlnet_scales_at; None: the first)."""
        arr = (ctypes.c_float * max(1, len(scales)))(*[float(v) for v in scales])
        if net is None:
            _hip.check(self._L.td_flux_set_controlnet_scales(self._h, ctypes.cast(arr, ctypes.c_void_p), len(scales)))
        else:
            _hip.check(self._L.td_flux_set_controlnet_scales_at(self._h, int(net), ctypes.cast(arr, ctypes.c_void_p), len(scales)))
        return self

    # ---- IP-Adapter (thinkdiff.models.flux_ip_adapter; td_flux_ip_adapter_*) ------------------------------------
    def ip_adapters(self) -> list:
        """The loaded adapters in load order: dicts of slot, num_tokens, embed_dim (the root's; forks share them)."""
        r = self._root()
        if not hasattr(r, "_ip_loaded"):
            r._ip_loaded = []
        return r._ip_loaded

    def load_ip_adapter(self, sd_or_path, weight_name: Optional[str] = None) -> int:
        """diffusers' `_load_ip_adapter_weights` for one adapter: a state dict (diffusers or XLabs keys), a local .safetensors file, or a
        directory + weight_name.  Adapters stack: the n-th call is adapter n of `set_ip_adapter_scale` / `set_ip_image_embeds`.  Its weights stay
        bf16 in every precision mode; scale 1.0 until set.  Returns the adapter's index."""
        from . import flux_ip_adapter as ipa
        if getattr(self, "_parent", None) is not None:
            raise _hip.ThinkDiffHipError("load_ip_adapter: adapters belong to the parent transformer (forks share its model)")
        c = self.config
        flat, num_tokens, embed_dim = ipa.load_ip_adapter_state_dict(sd_or_path, weight_name, num_layers=c.num_layers, joint_dim=c.joint_attention_dim,
                                                                     inner_dim=c.num_attention_heads * c.attention_head_dim)
        loaded = self.ip_adapters()
        if len(loaded) >= ipa.TD_IP_MAX_ADAPTERS:
            raise ValueError(f"load_ip_adapter: {ipa.TD_IP_MAX_ADAPTERS} adapters are loaded already (unload_ip_adapter first)")
        if num_tokens > ipa.TD_IP_MAX_KEYS:
            raise ValueError(f"load_ip_adapter: {num_tokens} tokens per image exceed the kernel's {ipa.TD_IP_MAX_KEYS} keys")
        slot = ctypes.c_int(-1)
        with torch.cuda.device(self.device):
            _hip.check(self._L.td_flux_ip_adapter_add(self._h, num_tokens, embed_dim, ctypes.byref(slot)))
            try:
                for name, t in flat.items():
                    d = t.to(self.device, torch.bfloat16).contiguous()
                    _OPS.flux_ip_adapter_load_param(int(self._h.value), slot.value, name, d)
                torch.cuda.current_stream().synchronize()      # `d` may be a temporary
            except Exception:
                self._L.td_flux_ip_adapter_remove(self._h, slot.value)      # no half-loaded adapter stays behind
                raise
        loaded.append(dict(slot=slot.value, num_tokens=num_tokens, embed_dim=embed_dim))
        return len(loaded) - 1

    def unload_ip_adapter(self):
        """diffusers' unload_ip_adapter: drop every adapter and this context's image prompts (forks: clear theirs with set_ip_image_embeds(None);
        a fork that still holds one refuses its forward and says so)."""
        if getattr(self, "_parent", None) is not None:
            raise _hip.ThinkDiffHipError("unload_ip_adapter: adapters belong to the parent transformer (forks share its model)")
        self.set_ip_image_embeds(None)
        _hip.check(self._L.td_flux_ip_adapter_remove(self._h, -1))
        self.ip_adapters().clear()

    def set_ip_adapter_scale(self, scale):
        """A float (all adapters, all double blocks) or a list with one entry per adapter, each a float or `num_layers` per-block floats."""
        from . import flux_ip_adapter as ipa
        loaded = self.ip_adapters()
        if not loaded:
            raise ValueError("set_ip_adapter_scale: no IP-Adapter is loaded (load_ip_adapter)")
        per = ipa.expand_scales(scale, len(loaded), self.config.num_layers)
        root = self._root()
        for a, s in zip(loaded, per):
            arr = (ctypes.c_float * len(s))(*s)
            _hip.check(self._L.td_flux_set_ip_adapter_scale(root._h, a["slot"], ctypes.cast(arr, ctypes.c_void_p), len(s)))

    def set_ip_image_embeds(self, embeds):
        """The image prompt of THIS context's image (forks hold their own): None clears; else one [n_img, E] tensor per adapter (a bare tensor with
        one adapter loaded).  Computes the image-prompt tokens and every double block's K / V once (td_flux_set_ip_image_embeds)."""
        loaded = self.ip_adapters()
        h = int(self._h.value)
        if embeds is None:
            for slot in range(4):
                _hip.check(self._L.td_flux_set_ip_image_embeds(self._h, slot, None, 0, None))
            return
        if not loaded:
            raise ValueError("set_ip_image_embeds: no IP-Adapter is loaded (load_ip_adapter)")
        if isinstance(embeds, torch.Tensor):
            embeds = [embeds]
        if len(embeds) != len(loaded):
            raise ValueError(f"set_ip_image_embeds: {len(embeds)} entries for {len(loaded)} loaded adapters")
        with torch.cuda.device(self.device):
            for a, e in zip(loaded, embeds):
                if e.dim() != 2 or e.shape[1] != a["embed_dim"]:
                    raise ValueError(f"set_ip_image_embeds: adapter {a['slot']} takes [n_img, {a['embed_dim']}], got {tuple(e.shape)}")
                d = e.to(self.device, torch.bfloat16).contiguous()
                _OPS.flux_set_ip_image_embeds(h, a["slot"], d)
            torch.cuda.current_stream().synchronize()      # `d` may be a temporary

    def read_ip(self, adapter: int, block: int = -1, which: int = 0) -> torch.Tensor:
        """Tests: this context's image-prompt tokens of adapter `adapter` (block < 0), or double block `block`'s K (which 0) / V (1)."""
        with torch.cuda.device(self.device):
            return _OPS.flux_ip_read(int(self._h.value), self.ip_adapters()[adapter]["slot"], int(block), int(which))

    # ---- per-launch HIP-event trace (bench.py roofline leg) ------------------------------------------
    TRACE_CATEGORIES = ("gemm_256x256", "gemm_other", "attention", "layernorm_modulate", "qk_rmsnorm_rope", "gemm_288x192")

    def trace_begin(self, max_launches: int):
        _hip.check(self._L.td_flux_trace_begin(self._h, max_launches))

    def trace_end(self):
        n = len(self.TRACE_CATEGORIES)
        counts, ms, fl = (ctypes.c_int64 * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
        _hip.check(self._L.td_flux_trace_end(self._h, _hip.stream_ptr(), ctypes.cast(counts, ctypes.c_void_p),
                                             ctypes.cast(ms, ctypes.c_void_p), ctypes.cast(fl, ctypes.c_void_p)))
        return {c: {"launches": int(counts[i]), "ms": float(ms[i]), "flops": float(fl[i])}
                for i, c in enumerate(self.TRACE_CATEGORIES)}

    # ---- diffusers-style call -------------------------------------------------------------------------
    def forward(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids=None,
                guidance=None, return_dict: bool = False, **_ignored):
        """[ext] FluxTransformer2DModel.forward semantics; batch is looped (conditions differ per sample).  A channel-conditioned model
        takes what diffusers passes it, hidden_states [B, S, in_channels] = cat(latents, condition), and splits it itself."""
        B = hidden_states.shape[0]
        outs = []
        c_lat, c_cond = self.config.latent_channels, self.config.cond_channels
        if hidden_states.shape[-1] != self.config.in_channels:
            raise ValueError(f"hidden_states has {hidden_states.shape[-1]} channels, the transformer's in_channels is {self.config.in_channels}")
        cond_all = hidden_states[..., c_lat:] if c_cond else None
        hidden_states = hidden_states[..., :c_lat]
        for b in range(B):
            self.set_condition(encoder_hidden_states[b], pooled_projections[b], img_ids, txt_ids)
            if c_cond:
                self.set_channel_condition(cond_all[b])
            t = float(timestep[b] if timestep.dim() else timestep)
            g = float(guidance[b] if guidance.dim() else guidance) if guidance is not None else 0.0
            # timestep arrives as t/1000 in the latents dtype; the transformer multiplies by 1000 in that dtype
            te = float((torch.tensor([t]).to(hidden_states.dtype) * 1000).float())
            ge = float((torch.tensor([g]).to(hidden_states.dtype) * 1000).float())
            self.set_timesteps([te], ge)
            outs.append(self.forward_step(hidden_states[b].to(torch.bfloat16).contiguous(), 0))
        out = torch.stack(outs)
        return (out,)

    __call__ = forward
